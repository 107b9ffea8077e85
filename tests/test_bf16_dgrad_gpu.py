"""The bf16 input gradient in one launch for any stride, with the fan-in fused (``zsv_conv3d_bf16_dgrad_pack`` +
``zsv_conv3d_bf16_dgrad``; ``Bf16TrainPath._dgrad``).

* exact bits through the raw ABI on the operands of ``bf16_exact_cases`` (fp32 accumulation is exact there: one correct bf16 code
  per output; ``test_bf16_dgrad_host.py`` checks the precondition of the added cases): without fan-in, with a separate fan-in
  buffer, with ``fanin == dx``, and at stride 1 on two routes;
* no behaviour change: on random bf16 operands ``_dgrad`` equals ``_dgrad_composed`` (the per-class composition it replaces) bit for
  bit, and with a fan-in it equals ``_dgrad_composed(...) + g``;
* the memory contract with guard bands around every buffer; the launch count from a kernel trace; one case at the benchmark's
  extents against float64.
"""
from ctypes import byref

import pytest
import torch

import bf16_exact_cases as X
import guarded as G
from test_bf16_dgrad_host import ALL_CASES, forward_desc

pytestmark = pytest.mark.gpu

import test_amp_full_size_gpu as FS  # noqa: E402  (its operand construction, channel sample and fp64 bar; its kernel trace)
from helpers import make_opt  # noqa: E402
from zeroshotvideoclassification_amd import _lib, amp, network, ops, synthetic  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
BY_NAME = {c.name: c for c in ALL_CASES}
STRIDED = [c for c in ALL_CASES if c.stride != (1, 1, 1)]


def _dev(t):
    return t.float().to(DEV)


def to_cl(t):
    return amp.ncdhw_to_cl_bf16(_dev(t))


def _dx_shape(case):
    n, cin, t, h, w = case.xs
    return (n, t, h, w, amp.channel_pitch(cin))


def _abi_dgrad(case, w, dz_cl, fanin=None, in_place=False):
    """pack + dgrad through the raw C ABI on the current (default) stream.  dx starts as NaN: an element nobody wrote shows."""
    lib = _lib.load()
    d = forward_desc(case)
    nb = int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(byref(d)))
    assert nb > 0
    blob = torch.empty(nb, dtype=torch.uint8, device=DEV)
    wd = _dev(w).contiguous()
    _lib.check(lib.zsv_conv3d_bf16_dgrad_pack(byref(d), wd.data_ptr(), blob.data_ptr(), ops._stream()), "pack")
    if in_place:
        dx = fanin.clone()
        fanin = dx
    else:
        dx = torch.full(_dx_shape(case), float("nan"), dtype=BF16, device=DEV)
    _lib.check(lib.zsv_conv3d_bf16_dgrad(byref(d), dz_cl.data_ptr(), blob.data_ptr(), ops._ptr(fanin), dx.data_ptr(), ops._stream()), "dgrad")
    torch.cuda.synchronize()
    return dx


_REF = {}


def _reference(case):
    """(w, dz, dx64, reached) of a case, computed once."""
    if case.name not in _REF:
        w, dz = X.dgrad_operands(case)
        dx64, total, reached = X.dgrad_reference(case, w, dz)
        X.assert_exact_in_fp32(X.DGRAD_Q, total + 3.0, w, dz)
        _REF[case.name] = (w, dz, dx64, reached)
    return _REF[case.name]


def _fanin(case):
    """bf16 values k/2, k in {-6..6}, (N, Cin, T, H, W) float64 on the host."""
    g = torch.Generator().manual_seed(len(case.name) + sum(case.xs))
    return torch.randint(-6, 7, tuple(case.xs), generator=g).double() / 2


def _check_exact(case, dx_cl, want, exact, what):
    cin = case.xs[1]
    got = X.channels_first(dx_cl, cin)
    assert tuple(got.shape) == tuple(case.xs)
    X.assert_same_values(got, want, exact, f"{case.name}: {what}")
    assert int(torch.count_nonzero(dx_cl[..., cin:].float())) == 0, "pad channels must be zero"


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_raw_abi_stores_the_one_correct_code(case):
    w, dz, dx64, reached = _reference(case)
    dx_cl = _abi_dgrad(case, w, to_cl(dz))
    _check_exact(case, dx_cl, X.rne_bf16(dx64), dx64, "dx")
    got = X.channels_first(dx_cl, case.xs[1])
    assert int(torch.count_nonzero(got.float()[~reached])) == 0, "a position no tap reaches must be exactly zero"


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_fan_in_is_added_to_the_rounded_gradient(case, in_place):
    """dx = bf16(float(bf16(acc)) + float(fanin)): the CPU's bf16 add of the rounded gradient and the fan-in."""
    w, dz, dx64, _ = _reference(case)
    f64 = _fanin(case)
    want = X.rne_bf16(dx64) + f64.to(BF16)
    assert want.dtype == BF16
    f_cl = to_cl(f64)
    before = f_cl.clone()
    dx_cl = _abi_dgrad(case, w, to_cl(dz), fanin=f_cl, in_place=in_place)
    _check_exact(case, dx_cl, want, dx64 + f64, "dx + fanin")
    assert torch.equal(f_cl, before), "a separate fan-in buffer is only read"


# stride-1 geometries small enough for the exact operands whose input-gradient problem reaches the shared-image kernel (144 rows,
# kW = 3) and the frames-x-positions kernel (64 rows, 8 frames x 32 positions): bf16_same_applicable / bf16_tsame_frames
ROUTE_CASES = {"s0": X.GradCase("s0", (1, 144, 2, 6, 6), 64, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
               "s1": X.GradCase("s1", (1, 45, 8, 8, 4), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0))}


@pytest.mark.parametrize("name,knob,kernel", [("s0", None, "conv_bf16_same_kernel<"), ("s1", None, "conv_bf16_tsame_kernel<"),
                                              ("s0", "ZSV_BF16_NO_SAME", "conv_bf16_kernel<")], ids=["same", "tsame", "NO_SAME-per_tap"])
def test_fan_in_at_stride_one_on_two_routes(name, knob, kernel, monkeypatch):
    """Stride 1 goes through the forward's kernel selection: the shared-image / frames-x-positions kernels by default, the per-tap
    kernel with the switch -- the round-then-add epilogue is the same code on each."""
    if knob:
        monkeypatch.setenv(knob, "1")
    case = ROUTE_CASES[name]
    w, dz, dx64, _ = _reference(case)
    f64 = _fanin(case)
    dz_cl, f_cl = to_cl(dz), to_cl(f64)
    names = FS._kernels_run(lambda: _abi_dgrad(case, w, dz_cl, fanin=f_cl))
    assert any(kernel in k for k in names), (kernel, sorted(k[:60] for k in names))
    assert not any("conv_bf16_dgrad_kernel" in k for k in names), "stride 1 runs the forward's kernels"
    for in_place in (False, True):
        dx_cl = _abi_dgrad(case, w, dz_cl, fanin=f_cl, in_place=in_place)
        _check_exact(case, dx_cl, X.rne_bf16(dx64) + f64.to(BF16), dx64 + f64, f"dx + fanin ({knob})")


def _record(case, seed):
    """(record, dz, g): a unit with random bf16-rounded weights, a random bf16 output gradient and fan-in (pad channels zero)."""
    n, cin, t, h, w_ = case.xs
    gen = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv3d(cin, case.cout, case.kernel, stride=case.stride, padding=case.padding, bias=False)
    fan = cin * case.kernel[0] * case.kernel[1] * case.kernel[2]
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=gen) * fan ** -0.5).to(BF16).float())
    u = amp._Unit(conv.to(DEV), torch.nn.BatchNorm3d(case.cout).to(DEV), False)
    rec = amp._Record()
    rec.unit, rec.desc = u, u.desc(n, t, h, w_)
    dz = to_cl(torch.randn((n, case.cout, rec.desc.To, rec.desc.Ho, rec.desc.Wo), generator=gen))
    g = to_cl(torch.randn(tuple(case.xs), generator=gen))
    return rec, dz, g


@pytest.mark.parametrize("case", STRIDED, ids=[c.name for c in STRIDED])
def test_no_behaviour_change_on_random_operands(case):
    """The K loop walks (tap, chunk) in the order of the per-tap kernel run per class, so the fp32 sums are the same numbers:
    ``torch.equal``, not a tolerance."""
    rec, dz, g = _record(case, 1234 + len(case.name))
    composed = amp.Bf16TrainPath._dgrad_composed(rec, dz)
    assert torch.equal(amp.Bf16TrainPath._dgrad(rec, dz), composed)
    assert torch.equal(amp.Bf16TrainPath._dgrad(rec, dz, fanin=g), composed + g)
    acc = g.clone()
    out = amp.Bf16TrainPath._dgrad(rec, dz, fanin=acc, out=acc)
    assert out is acc and torch.equal(acc, composed + g)


@pytest.mark.parametrize("name", ["d2", "d4", "d7", "x1"])
def test_memory_contract(name):
    """dz, the forward weight, the blob, the fan-in and dx in buffers of exactly their size between guard bands: nothing is written
    outside blob and dx, every element of dx is written (0xFF prefill), and the result does not depend on the bytes around the
    inputs (two poison bytes) nor on the blob's prefill."""
    case = BY_NAME[name]
    lib = _lib.load()
    d = forward_desc(case)
    w, dz, _, _ = _reference(case)
    wd, dz_cl, f_cl = _dev(w).contiguous(), to_cl(dz), to_cl(_fanin(case))
    nb = int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(byref(d)))
    shape = _dx_shape(case)
    for fanin in (None, f_cl):
        want = _abi_dgrad(case, w, dz_cl, fanin=fanin)
        for band, fill in zip(G.BAND_BYTES, G.FILLS):
            ins = {k: G.guarded_copy(v, DEV, guard_byte=band) for k, v in (("w", wd), ("dz", dz_cl), ("fanin", f_cl))}
            blob = G.guarded(nb, DEV, fill)
            dx = G.guarded_like(BF16, shape, DEV, 0xFF)
            _lib.check(lib.zsv_conv3d_bf16_dgrad_pack(byref(d), ins["w"].ptr, blob.ptr, ops._stream()), "pack")
            _lib.check(lib.zsv_conv3d_bf16_dgrad(byref(d), ins["dz"].ptr, blob.ptr, ins["fanin"].ptr if fanin is not None else None,
                                                 dx.ptr, ops._stream()), "dgrad")
            torch.cuda.synchronize()
            for k, b in list(ins.items()) + [("blob", blob), ("dx", dx)]:
                b.check(f"{name}: {k}")
            for k, v in (("w", wd), ("dz", dz_cl), ("fanin", f_cl)):
                assert torch.equal(ins[k].payload, v.reshape(-1).view(torch.uint8)), f"{k} is only read"
            got = dx.view(BF16, shape)
            G.assert_all_written(got, f"{name}: dx")
            assert torch.equal(got, want), f"{name}: the result depends on bytes outside the inputs (band 0x{band:02X}) or on the blob's prefill"


def _kernel_counts(fn):
    """{kernel name without spaces: launches} of ``fn``, from a kernel trace: the events that ran on the device (kernels, and any
    copy or fill), not the runtime calls that enqueued them."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key.replace(" ", ""): e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA}


@pytest.mark.parametrize("name", ["d2", "d3", "d4", "d6"])
def test_strided_input_gradient_with_fan_in_is_two_launches(name):
    rec, dz, g = _record(BY_NAME[name], 77)
    amp.Bf16TrainPath._dgrad(rec, dz, fanin=g)                     # (module load, function attributes)
    torch.cuda.synchronize()
    counts = _kernel_counts(lambda: amp.Bf16TrainPath._dgrad(rec, dz, fanin=g))
    assert sum(counts.values()) == 2, counts
    assert any("pack_bf16_dgrad_kernel" in k for k in counts) and any("conv_bf16_dgrad_kernel" in k for k in counts), counts
    assert not any("at::native" in k for k in counts), counts


# torch kernels of a backward that come from neither ``_dgrad`` nor the residual joins (none is known today; a name added here
# needs a comment saying where it is launched)
BACKWARD_TORCH_KERNELS_ALLOWED = ()


def _trunk(frames):
    """(path, run): an r2plus1d_18 trunk in train mode; ``run()`` = (tape of a forward of 2 x 3 x frames x 32 x 32, a random dfeat)."""
    model = network.get_network(make_opt("r2plus1d_18"))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model = model.to(DEV).train()
    path = amp.Bf16TrainPath(model.model)
    clips = synthetic.synthetic_clips(2, frames, 32)[:, 0].contiguous().to(DEV)
    assert tuple(clips.shape) == (2, 3, frames, 32, 32)

    def run():
        tape = []
        feat = path.forward(clips, tape)
        gen = torch.Generator().manual_seed(5)
        dfeat = to_cl(torch.randn((feat.shape[0], path.features) + tuple(feat.shape[1:4]), generator=gen))
        torch.cuda.synchronize()
        return tape, dfeat

    return path, run


def test_backward_of_the_trunk_runs_no_torch_kernel():
    path, run = _trunk(4)
    tape, dfeat = run()
    path.backward(tape, dfeat)                                      # warm-up: module load, workspaces, side streams
    ops.join_wgrad_streams()
    tape, dfeat = run()
    grads = {}

    def backward():
        grads.update(path.backward(tape, dfeat))
        ops.join_wgrad_streams()

    counts = _kernel_counts(backward)
    torch_kernels = sorted(k for k in counts if "at::native" in k and not any(a in k for a in BACKWARD_TORCH_KERNELS_ALLOWED))
    assert not torch_kernels, torch_kernels
    strided = sum(1 for u in path.units[len(path.stem):] if u.stride != (1, 1, 1))
    assert sum(n for k, n in counts.items() if "conv_bf16_dgrad_kernel" in k) == strided == 9, counts
    assert len(grads) == len(path.params) and all(bool(torch.isfinite(v).all()) for v in grads.values())


def test_backward_gradients_are_those_of_the_composed_path():
    """The ``grads`` dict of ``Bf16TrainPath.backward`` bit for bit against the same walk with the per-class composition and torch
    joins (what it did before).  8 frames: the composition does not take a strided axis of extent 1 (layer4 at 4 frames)."""
    path, run = _trunk(8)
    tape, dfeat = run()
    grads = path.backward(tape, dfeat)
    ops.join_wgrad_streams()
    tape2, _ = run()
    fused = amp.Bf16TrainPath._dgrad

    def composed(r, dz, fanin=None, out=None):
        dx = amp.Bf16TrainPath._dgrad_composed(r, dz)
        return dx if fanin is None else dx + fanin

    amp.Bf16TrainPath._dgrad = staticmethod(composed)
    try:
        want = path.backward(tape2, dfeat)
        ops.join_wgrad_streams()
    finally:
        amp.Bf16TrainPath._dgrad = staticmethod(fused)
    torch.cuda.synchronize()
    assert want.keys() == grads.keys() and len(grads) == len(path.params)
    for k in want:
        assert torch.equal(want[k], grads[k]), "a parameter gradient moved"


def test_layer2_entry_at_the_benchmark_extents():
    """Input (2, 64, 16, 56, 56) -> 230, (1,3,3), stride (1,2,2): layer2's entry with 2 clips.  The operand construction, the channel
    sample and the bar of ``test_input_gradient_at_size`` (2^-7 of the range against float64 of the bf16-rounded operands), and bit
    for bit the composition."""
    n, cin, cout, (t, h, w), k, s, p = 2, 64, 230, (16, 56, 56), (1, 3, 3), (1, 2, 2), (0, 1, 1)
    seed = 4242
    wgt = FS._randn((cout, cin) + k, seed + 1, (cin * 9) ** -0.5)
    conv = torch.nn.Conv3d(cin, cout, k, stride=s, padding=p, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wgt)
    u = amp._Unit(conv, torch.nn.BatchNorm3d(cout).to(DEV), False)
    rec = amp._Record()
    rec.unit, rec.desc = u, u.desc(n, t, h, w)
    out = FS._out_dims(t, h, w, k, s, p)
    dz = FS._randn((n, cout) + out, seed + 3)
    dz_cl = amp.ncdhw_to_cl_bf16(dz)
    dx_cl = amp.Bf16TrainPath._dgrad(rec, dz_cl)
    torch.cuda.synchronize()
    assert tuple(dx_cl.shape) == (n, t, h, w, 64)
    chans = FS._channels(cin, 24, 7)
    ref = torch.nn.grad.conv3d_input((n, len(chans), t, h, w), wgt[:, chans].double().cpu(), dz.double().cpu(), s, p)
    got = FS._cl_sample(dx_cl, range(n), chans)
    assert float((got - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -7
    assert torch.equal(dx_cl, amp.Bf16TrainPath._dgrad_composed(rec, dz_cl))
    g = amp.ncdhw_to_cl_bf16(FS._randn((n, cin, t, h, w), seed + 4))
    assert torch.equal(amp.Bf16TrainPath._dgrad(rec, dz_cl, fanin=g), dx_cl + g)
