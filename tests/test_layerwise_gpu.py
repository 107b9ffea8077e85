"""``optim.FusedLARS`` / ``optim.FusedLAMB`` (csrc/layerwise.hip) on the device against the fp64 restatement of
tests/layerwise_cases.py.

Bars.  Parameters: ``BAR * max|ref|`` per tensor after every step, ``BAR = 2e-6``, the bar of tests/test_optim_decay_clip_gpu.py.
Trust ratios (``layer_norms[:, 2]``): ``BAR`` relative.  Worst case: a chunk sum is 16 serial adds and an 8-level tree, 24 roundings
of a positive sum, plus the double sum's rounding to fp32: 25 * 2^-24 = 1.5e-6 on a sum of squares, halved by the square root, for two
norms, plus the fp32 rounding of ``u``: about 1.7e-6.  The same rules in torch float32 on the CPU stay within 3.7e-7 (parameters)
and 7.9e-7 (ratios) of the fp64 run on these cases.  The two norms of a record are held to the same bar (each carries half of it).
The exact cases are bit for bit."""
import copy
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G  # noqa: E402
import layerwise_cases as C  # noqa: E402
import stalled  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ddp, network, optim, resnet, train  # noqa: E402

DEV = "cuda"
KINDS = ("lars", "lamb")
CLS = {"lars": optim.FusedLARS, "lamb": optim.FusedLAMB}
EPS = 2.0 ** -23


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _build(kind, ps, groups, **kw):
    """Parameters on the device and the optimizer over ``groups`` ([(indices, group options)], tests/layerwise_cases.py)."""
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    spec = [dict(hp, params=[params[i] for i in indices]) for indices, hp in groups]
    if kind == "lars":
        kw.setdefault("lr", groups[0][1]["lr"])
    return params, CLS[kind](spec, **kw)


def _order(groups):
    return [i for indices, _ in groups for i in indices]


def _check_step(params, opt, groups, want, what):
    """Parameters within BAR * max|ref|, records within BAR relative; the figures are printed before anything is asserted."""
    p64, rec64, _ = want
    worst_p = max(((params[i].detach().double().cpu() - p64[i]).abs().max().item() / p64[i].abs().max().item(), i)
                  for i in range(len(params)) if p64[i].abs().max().item() > 0)
    got = opt.layer_norms.double().cpu()
    ref = torch.tensor(rec64, dtype=torch.float64)
    assert got.shape == ref.shape and [id(p) for p in opt.layer_params] == [id(params[i]) for i in _order(groups)]
    rel = (got - ref).abs() / ref.abs().clamp_min(1e-300)
    rel[ref == 0] = (got - ref).abs()[ref == 0]                # a zero norm must be zero
    print(f"{what}: parameters {worst_p[0]:.3e} (tensor {worst_p[1]}), |p| {rel[:, 0].max():.3e}, |q| {rel[:, 1].max():.3e}, "
          f"ratio {rel[:, 2].max():.3e}; bar {C.BAR:.1e}")
    assert worst_p[0] <= C.BAR, (what, worst_p)
    assert rel[:, 2].max().item() <= C.BAR, (what, "ratio", int(rel[:, 2].argmax()), rel[:, 2].max().item())
    assert rel[:, :2].max().item() <= C.BAR, (what, "norms", rel[:, :2].max().item())


def _steps(params, opt, grads, scaler=None, scale=1.0):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = (g * scale).to(DEV)
        if scaler is None:
            opt.step()
        else:
            scaler.step(opt)
            scaler.update()


# ---- 1: parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_fp64_rule(kind, case):
    """1: five steps; chunk edges, a tensor of 301 chunks, a zero tensor and a zero gradient (sizes); 70 tensors whose norms are
    1 .. 70 in two groups, one of them with adapt=False (many): a ratio that lands on the wrong tensor is an error of order 1."""
    make, groups = C.CASES[case]
    ps, grads = make()
    groups = groups(kind)
    params, opt = _build(kind, ps, groups)
    ref = C.reference(kind, case)
    for step in range(C.STEPS):
        _steps(params, opt, grads[step:step + 1])
        _check_step(params, opt, groups, ref[step], f"{kind} {case} step {step + 1}")
    for i, p in enumerate(params):
        state = opt.state[p]
        assert set(state) == ({"momentum_buffer"} if kind == "lars" else {"step", "exp_avg", "exp_avg_sq"}), i
        if kind == "lamb":
            assert float(state["step"]) == C.STEPS


# ---- 2: exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.EXACT_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_cases_bit_for_bit(kind, n):
    """2: p = 2, g = 1 over one and four chunks; every intermediate is a power of two."""
    ps, grads = C.exact_case(n)
    groups = C.exact_groups(kind)
    (p64, rec64, state64), = C.run(kind, ps, grads, groups)
    params, opt = _build(kind, ps, groups)
    _steps(params, opt, grads)
    _same(params[0], p64[0].float().to(DEV), f"{kind} n={n} parameters")
    assert float(params[0].detach()[0]) == C.EXACT_AFTER[kind]
    _same(opt.layer_norms, torch.tensor(rec64, dtype=torch.float32, device=DEV), f"{kind} n={n} records")
    keys = ("momentum_buffer",) if kind == "lars" else ("exp_avg", "exp_avg_sq")
    for k, want in zip(keys, state64[0]):
        _same(opt.state[params[0]][k], want.float().to(DEV), f"{kind} n={n} {k}")


# ---- 3: adapt=False is FusedSGD ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", [dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-2),
                                dict(momentum=0.8, dampening=0.5, nesterov=False, weight_decay=1e-3, maximize=True)],
                         ids=["nesterov", "dampening-maximize"])
def test_lars_without_adaptation_is_fused_sgd_bit_for_bit(hp):
    """3: three steps; parameters and momentum buffers carry FusedSGD's bits, and every recorded ratio is 1."""
    ps, grads = C.sizes_case()
    a = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    b = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    lars = optim.FusedLARS([dict(params=a, adapt=False)], lr=0.05, **hp)
    sgd = optim.FusedSGD(b, lr=0.05, **hp)
    for gs in grads[:3]:
        _steps(a, lars, [gs])
        _steps(b, sgd, [gs])
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"parameter {i}")
            _same(lars.state[x]["momentum_buffer"], sgd.state[y]["momentum_buffer"], f"buffer {i}")
    assert bool((lars.layer_norms[:, 2] == 1).all())


# ---- 4: the loss scaler --------------------------------------------------------------------------------------------------------------
def _inject_workspace(opt, chunks, count, fill):
    """A workspace of the queried size holding ``fill`` in every float, handed to the optimizer before its first step."""
    nbytes = int(_lib.load().zsv_layerwise_workspace_bytes(chunks, count))
    opt._layer_ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device=DEV)
    return opt._layer_ws


@pytest.mark.parametrize("kind", KINDS)
def test_under_the_loss_scaler(kind):
    """4: scale 65536.  Step 0 carries one inf: parameters, moments / buffers, shadows and the records keep their bits.  Step 1 is
    then the first (LARS with dampening 0.5: buf = d; LAMB: t = 1), held to the fp64 rule that skips step 0, and the scaled run
    stays within BAR of an unscaled one.  The last step (every slot of the table ring has been used by then) is queued behind a
    stalled stream: the host does not wait for the device."""
    ps, grads = C.sizes_case()
    groups = C.sizes_groups(kind)
    if kind == "lars":
        groups = [(groups[0][0], dict(groups[0][1], dampening=0.5))]
    chunks = sum((n + C.CHUNK - 1) // C.CHUNK for n in C.SIZES)
    params, opt = _build(kind, ps, groups)
    avg = optim.WeightAverage(opt, decay=0.9)
    ws = _inject_workspace(opt, chunks, len(ps), 7.0)
    scaler = optim.LossScaler(init_scale=65536.0)
    start = [p.detach().clone() for p in params]
    poisoned = [g.clone() for g in grads[0]]
    poisoned[5][17] = float("inf")
    _steps(params, opt, [poisoned], scaler, 65536.0)
    keys = ("momentum_buffer",) if kind == "lars" else ("exp_avg", "exp_avg_sq")
    for i, (p, p0) in enumerate(zip(params, start)):
        _same(p, p0, f"skipped step: parameter {i}")
        for k in keys:
            assert not bool(opt.state[p][k].any()), (i, k)
    for (k, s), p0 in zip(avg.shadows().items(), start):
        _same(s, p0, f"skipped step: shadow {k}")
    assert bool((ws == 7.0).all()), "a skipped step wrote the workspace"
    assert opt._layer_ws is ws and int(avg.n_averaged) == 0
    st = scaler.state()
    assert st["scale"] == 32768.0 and st["steps_done"] == 0
    # steps 1 .. 4 are the first .. fourth taken steps
    want = C.run(kind, ps, grads, groups, skipped={0})
    _steps(params, opt, grads[1:2], scaler, 32768.0)
    _check_step(params, opt, groups, want[1], f"{kind} scaled, first taken step")
    _steps(params, opt, grads[2:4], scaler, 32768.0)
    scaled = [(g * 32768.0).to(DEV) for g in grads[4]]
    torch.cuda.synchronize()
    held = stalled.stall(torch.cuda.current_stream(), stalled.STALL_MS)
    for p, g in zip(params, scaled):
        p.grad = g
    scaler.step(opt)
    scaler.update()
    assert stalled.held(held), "the step waited for the device (or the stall was too short to tell)"
    torch.cuda.synchronize()
    _check_step(params, opt, groups, want[4], f"{kind} scaled, fourth taken step")
    assert scaler.state()["steps_done"] == 4 and int(avg.n_averaged) == 4
    # the unscaled run of the same four steps
    plain, plain_opt = _build(kind, ps, groups)
    _steps(plain, plain_opt, grads[1:5])
    for i, (x, y) in enumerate(zip(params, plain)):
        err, bound = (x.detach() - y.detach()).abs().max().item(), C.BAR * y.detach().abs().max().item()
        assert err <= bound, ("scaled against unscaled", i, err, bound)


# ---- 5: clipping ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_max_grad_norm_precedes_the_moments_and_the_norms(kind):
    """5: the total norm of the sizes case is about 11, max_grad_norm 4: every step is clipped; the fp64 rule gets
    g * min(1, max / (norm + 1e-6)) and the device has to agree on parameters, gradient / update norms and ratios."""
    ps, grads = C.sizes_case()
    grads = grads[:3]
    groups = C.sizes_groups(kind)
    max_norm = 4.0
    norms = [torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).item() for gs in grads]
    assert all(n > max_norm for n in norms)
    want = C.run(kind, ps, grads, groups, coefs=[max_norm / (n + 1e-6) for n in norms])
    params, opt = _build(kind, ps, groups, max_grad_norm=max_norm)
    for step, gs in enumerate(grads):
        _steps(params, opt, [gs])
        got = opt.grad_norm
        assert got.is_cuda and got.dim() == 0
        rel = abs(got.item() - norms[step]) / norms[step]
        print(f"{kind} step {step + 1}: grad_norm {got.item():.6f} fp64 {norms[step]:.6f} rel {rel:.3e}")
        assert rel <= C.BAR
        _check_step(params, opt, groups, want[step], f"{kind} clipped step {step + 1}")
        for p, g in zip(params, gs):
            _same(p.grad, g.to(DEV), ".grad is not rewritten")


# ---- 6: the weight average --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.9, None], ids=["ema", "equal-weight"])
@pytest.mark.parametrize("kind", KINDS)
def test_weight_average_follows_the_new_parameters(kind, decay):
    """6: after every taken step the shadow is lerp(shadow, new p, w) -- a copy on the first averaged step -- to the 3 * 2^-23 of
    tests/test_weight_average_gpu.py (two roundings of the lerp); a step the scaler skips (the second) averages nothing."""
    ps, grads = C.many_case()
    grads = [[g.clone() for g in gs] for gs in grads[:4]]
    grads[1][3][0] = float("nan")
    groups = C.many_groups(kind)
    params, opt = _build(kind, ps, groups)
    avg = optim.WeightAverage(opt, decay=decay)
    scaler = optim.LossScaler(init_scale=4.0)
    averaged = 0
    for step, gs in enumerate(grads):
        before = [s.clone() for s in avg.shadows().values()]
        old = [p.detach().clone() for p in params]
        _steps(params, opt, [gs], scaler, scaler.get_scale())
        if step == 1:
            for s, b, p, o in zip(avg.shadows().values(), before, params, old):
                _same(s, b, "skipped step: shadow")
                _same(p, o, "skipped step: parameter")
            assert int(avg.n_averaged) == averaged
            continue
        w = (1.0 - decay) if decay is not None else 1.0 / (averaged + 1)
        for i, (s, b, p) in enumerate(zip(avg.shadows().values(), before, params)):
            assert not torch.equal(p.detach(), old[i]), i
            if averaged == 0:
                _same(s, p, f"first averaged step copies ({i})")
                continue
            ref = torch.lerp(b.double(), p.detach().double(), w)
            bound = 3 * EPS * max(b.abs().max().item(), p.detach().abs().max().item())
            assert (s.double() - ref).abs().max().item() <= bound, (step, i)
        averaged += 1
        assert int(avg.n_averaged) == averaged
    assert averaged == 3


# ---- 7, 11: the model ----------------------------------------------------------------------------------------------------------------------
def _small_model(seed=31):
    torch.manual_seed(seed)
    trunk = lambda pretrained=False: resnet.VideoResNet(resnet.BasicBlock, [resnet.Conv2Plus1D] * 4, [1, 1, 1, 1],  # noqa: E731
                                                        resnet.R2Plus1dStem)
    return network.Model(trunk).to(DEV).train()


def _batch():
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(2, 1, 3, 4, 32, 32, generator=gen).to(DEV)
    z = torch.nn.functional.normalize(torch.randn(2, 300, generator=gen)).to(DEV)
    return x, z


def _make_opt(kind, params, **kw):
    return optim.FusedLARS(params, lr=0.05, **kw) if kind == "lars" else optim.FusedLAMB(params, lr=1e-3, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_bucket_path_matches_the_per_step_tables(kind):
    """7: GradientSync(local=True) + grad_buckets= on the [1, 1, 1, 1] trunk: from the moment the buckets exist the table is the
    static one, the states are views of flat buffers laid out like the buckets, and parameters, states and records carry the bits
    of a twin stepped through per-step tables (bucket slices start at arbitrary element offsets: the 4-byte forms of the kernels)."""
    x, z = _batch()
    crit = torch.nn.MSELoss()
    model = _small_model()
    sync = ddp.GradientSync(model, bucket_bytes=200 * 1024, local=True)
    opt = _make_opt(kind, model.parameters(), grad_buckets=sync)
    for _ in range(3):
        train.train_step(model, opt, crit, x, z, sync)
    assert sync.ready and opt._static is not None and opt._static[0] == sync.layout_version and len(sync.bucket_layout()) >= 2
    keys = opt._state_keys(opt.param_groups[0])
    for (flat, rows), state_flats in zip(sync.bucket_layout(), opt._static[5]):
        for p, off in rows:
            for k, f in zip(keys, state_flats):
                assert opt.state[p][k].data_ptr() == f.data_ptr() + 4 * off
    records = {id(p): r.clone() for p, r in zip(opt.layer_params, opt.layer_norms)}
    sync.remove()
    twin = _small_model()
    twin_opt = _make_opt(kind, twin.parameters())
    for _ in range(3):
        train.train_step(twin, twin_opt, crit, x, z)
    assert twin_opt._static is None
    twin_records = {id(p): r for p, r in zip(twin_opt.layer_params, twin_opt.layer_norms)}
    assert len(records) == len(twin_records)
    for (k, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        _same(p, q, k)
        if p.grad is not None:
            for key in keys:
                _same(opt.state[p][key], twin_opt.state[q][key], f"{k} {key}")
            _same(records[id(p)], twin_records[id(q)], f"{k} record")


@pytest.mark.parametrize("kind", KINDS)
def test_model_level_training_steps(kind):
    """11: network.Model over the [1, 1, 1, 1] R(2+1)D trunk, 2 clips of 3x4x32x32, three train_steps on layerwise_groups."""
    x, z = _batch()
    model = _small_model()
    groups = optim.layerwise_groups(model, 1e-4 if kind == "lars" else 0.01)
    opt = _make_opt(kind, groups)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    for _ in range(3):
        y, loss = train.train_step(model, opt, torch.nn.MSELoss(), x, z)
        assert bool(torch.isfinite(loss))
    live = 0
    for k, p in model.named_parameters():
        if p.grad is None:                                     # the encoder the forward never applies, and the trunk's fc
            assert torch.equal(p.detach(), before[k]) and not opt.state[p], k
            continue
        live += 1
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k
    dead = [k for k, p in model.named_parameters() if p.grad is None]
    assert any(k.startswith("encoder.") for k in dead) and live > 0
    norms = opt.layer_norms
    assert tuple(norms.shape) == (live, 3) and len(opt.layer_params) == live and bool(torch.isfinite(norms).all())
    adapt = torch.tensor([p.dim() >= 2 for p in opt.layer_params], device=DEV)
    assert bool((norms[~adapt, 2] == 1).all()) and bool((norms[adapt, 2] != 1).all())


# ---- 8, 9: the raw entry points: alignment and the workspace's bands ------------------------------------------------------------------
RAW_SIZES = C.SIZES[:8]


def _held(values, shift):
    """A copy of ``values`` that starts ``shift`` elements past a 256-byte boundary."""
    base = torch.empty(values.numel() + 64, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 256 == 0
    view = base[shift:shift + values.numel()]
    view.copy_(values)
    return view


def _raw_step(kind, shift, workspace=None):
    """One step that is not the first through the C ABI: p, g, both states and an EMA shadow of every tensor are views ``shift``
    elements past a 256-byte boundary.  Returns (parameters, first state, second state, shadows, records)."""
    lib = _lib.load()
    ps, grads = C.sizes_case()
    gen = torch.Generator().manual_seed(77)
    held, rows, first = [], [], 0
    for i, n in enumerate(RAW_SIZES):
        s1 = 0.01 * torch.randn(n, generator=gen)
        s2 = 1e-4 * torch.rand(n, generator=gen)
        arrays = [_held(t, shift) for t in (ps[i], grads[1][i], s1, s2, ps[i] * 0.5)]
        assert all(a.data_ptr() % 16 == 4 * shift for a in arrays)
        held.append(arrays)
        rows.append((arrays[0].data_ptr(), arrays[1].data_ptr(), arrays[2].data_ptr(), arrays[3].data_ptr(), n, first))
        first += (n + C.CHUNK - 1) // C.CHUNK
    count = len(rows)
    table = torch.frombuffer(bytearray(b"".join(struct.pack("<QQQQqq", *r) for r in rows)), dtype=torch.uint8).to(DEV)
    shadows = torch.tensor([a[4].data_ptr() for a in held], dtype=torch.int64, device=DEV)
    avg_state = torch.tensor([1], dtype=torch.int32, device=DEV)
    nbytes = int(lib.zsv_layerwise_workspace_bytes(first, count))
    assert nbytes % 4 == 0
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=DEV) if workspace is None else workspace(nbytes)
    ws_ptr = ws.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    place = (table.data_ptr(), count, first, 0, 0, count, ws_ptr, nbytes)
    if kind == "lars":
        hp = C.LARS_HP
        status = [lib.zsv_lars_norms(*place, None, stream),
                  lib.zsv_layerwise_finalize(*place, 0, 1, hp["trust_coefficient"], hp["weight_decay"], hp["eps"], 0.0, None, None, 0, stream),
                  lib.zsv_lars_multi(table.data_ptr(), count, first, ws_ptr, hp["lr"], hp["momentum"], 0.5, 0, hp["weight_decay"], 0, None,
                                     None, 0, -1, shadows.data_ptr(), avg_state.data_ptr(), 0.25, stream)]
    else:
        hp = C.LAMB_HP
        b1, b2 = hp["betas"]
        status = [lib.zsv_lamb_moments(*place, b1, b2, hp["eps"], hp["weight_decay"], None, None, 0, 3, stream),
                  lib.zsv_layerwise_finalize(*place, 1, 1, 0.0, 0.0, 0.0, 0.0, None, None, 0, stream),
                  lib.zsv_lamb_multi(table.data_ptr(), count, first, ws_ptr, hp["lr"], b1, b2, hp["eps"], hp["weight_decay"], None, 3,
                                     shadows.data_ptr(), avg_state.data_ptr(), 0.25, stream)]
    torch.cuda.synchronize()
    assert status == [0, 0, 0], status
    return [[a[j].clone() for a in held] for j in (0, 2, 3, 4)] + [ws[:3 * count].clone().view(count, 3)]


def _raw_equal(a, b, what):
    names = ("parameters", "first state", "second state", "shadows")
    for name, xs, ys in zip(names, a[:4], b[:4]):
        for i, (x, y) in enumerate(zip(xs, ys)):
            _same(x, y, f"{what}: {name} of tensor {i} (n = {RAW_SIZES[i]})")
    _same(a[4], b[4], f"{what}: records")


@pytest.mark.parametrize("kind", KINDS)
def test_element_aligned_tensors_give_the_same_bits(kind):
    """8: p, g, states and shadows one element past a 16-byte boundary (the 4-byte form of every array) against the same step on
    16-byte boundaries: equal bits -- sums included, since which lane adds which element does not depend on the form."""
    aligned = _raw_step(kind, 0)
    assert not torch.equal(aligned[0][-1], C.sizes_case()[0][len(RAW_SIZES) - 1].to(DEV))      # the step moved something
    _raw_equal(aligned, _raw_step(kind, 1), f"{kind} +4 bytes")
    _raw_equal(aligned, _raw_step(kind, 3), f"{kind} +12 bytes")


@pytest.mark.parametrize("kind", KINDS)
def test_workspace_stays_inside_its_guard_bands(kind):
    """9: records and partials in a workspace of exactly the queried size between two guard bands, prefilled with NaN: the bands
    stay intact, no NaN reaches a result, and NaN bands (0xFF) change no bit -- nothing outside the workspace is read."""
    plain = _raw_step(kind, 0)
    for band in (G.GUARD_BYTE, 0xFF):
        box = {}

        def workspace(nbytes):
            box["g"] = G.guarded(nbytes, DEV, 0xFF, guard_byte=band)
            return box["g"].view(torch.float32, (nbytes // 4,))

        got = _raw_step(kind, 0, workspace)
        box["g"].check(f"{kind} workspace, bands 0x{band:02X}")
        assert not bool(torch.isnan(got[4]).any())
        _raw_equal(plain, got, f"{kind} guarded workspace, bands 0x{band:02X}")


# ---- 10: reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_equal_bits(kind):
    ps, grads = C.sizes_case()
    runs = []
    for _ in range(2):
        params, opt = _build(kind, ps, C.sizes_groups(kind))
        _steps(params, opt, grads[:2])
        runs.append(([p.detach().clone() for p in params], opt.layer_norms.clone()))
    for i, (x, y) in enumerate(zip(runs[0][0], runs[1][0])):
        _same(x, y, f"parameter {i}")
    _same(runs[0][1], runs[1][1], "records")


# ---- 12: state dicts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_continues_bit_identically(kind):
    ps, grads = C.many_case()
    groups = C.many_groups(kind)
    params, opt = _build(kind, ps, groups)
    _steps(params, opt, grads[:2])
    saved = copy.deepcopy(opt.state_dict())
    twins, fresh = _build(kind, [p.detach().cpu() for p in params], groups)
    fresh.load_state_dict(saved)
    _steps(params, opt, grads[2:4])
    _steps(twins, fresh, grads[2:4])
    for i, (x, y) in enumerate(zip(params, twins)):
        _same(x, y, f"parameter {i}")
    _same(opt.layer_norms, fresh.layer_norms, "records")
    _check_step(twins, fresh, groups, C.reference(kind, "many")[3], f"{kind} resumed")


def test_a_fused_adam_state_loads_into_fused_lamb():
    """12: two FusedAdam steps, then FusedLAMB continues from that state: t = 3 and Adam's moments, held to the fp64 rule.

    The rule continues here from moments the DEVICE formed, and the C ABI takes the betas as fp32: (float)0.999 is 0.999 + 1.3e-8,
    which is 1.3e-5 of 1 - beta2.  A run from zero moments does not see that -- v and 1 - beta2^t carry the same factor, as in
    FusedAdam -- but a continuation with the exact 0.999 would mix the two (4e-6 on |u| at t = 3), so the fp64 continuation
    takes the betas rounded to fp32, which is what the loaded moments were formed with."""
    ps, grads = C.many_case()
    a = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    adam = optim.FusedAdam(a, lr=1e-3)
    _steps(a, adam, grads[:2])
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    lamb = optim.FusedLAMB(b, trust_clip=5.0)
    lamb.load_state_dict(copy.deepcopy(adam.state_dict()))
    hp = dict(C.LAMB_HP, lr=1e-3, eps=1e-8, weight_decay=0.0, trust_clip=5.0)            # Adam's group options, LAMB's own clip
    assert {k: lamb.param_groups[0][k] for k in hp} == hp and lamb.param_groups[0]["adapt"] is True
    _steps(b, lamb, grads[2:3])
    hp["betas"] = tuple(torch.tensor(hp["betas"], dtype=torch.float32).double().tolist())
    for i, (x, y) in enumerate(zip(a, b)):
        st = adam.state[x]
        want, _, _, rec = C.lamb_step(x.detach().double().cpu(), grads[2][i].double(), st["exp_avg"].double().cpu(),
                                      st["exp_avg_sq"].double().cpu(), 3, hp)
        err = (y.detach().double().cpu() - want).abs().max().item()
        assert err <= C.BAR * want.abs().max().item(), (i, err)
        assert abs(lamb.layer_norms[i, 2].item() - rec[2]) <= C.BAR * rec[2], (i, rec)
        assert float(lamb.state[y]["step"]) == 3


# ---- what existed launches what it launched ---------------------------------------------------------------------------------------------------
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


def test_launches_of_every_optimizer(monkeypatch):
    """FusedAdam.step() and FusedSGD.step() call what they called before this file's optimizers existed -- one update launch per
    group, the norm pair with max_grad_norm -- and none of the new entry points; FusedLARS / FusedLAMB call three per group."""
    names = [n for n in _lib.SIGNATURES if n.startswith(("zsv_adam", "zsv_sgd", "zsv_grad_", "zsv_lars", "zsv_lamb", "zsv_layerwise", "zsv_avg",
                                                         "zsv_scaler")) and not n.endswith("_workspace_bytes")]        # launches, not queries
    calls = _count(monkeypatch, names)

    def stepped(make):
        ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 5000)]
        opt = make([dict(params=ps[:1]), dict(params=ps[1:])])
        for p in ps:
            p.grad = torch.randn_like(p)
        for n in calls:
            calls[n] = 0
        opt.step()
        return {n: c for n, c in calls.items() if c}

    assert stepped(lambda g: optim.FusedAdam(g, lr=1e-3)) == {"zsv_adam_multi": 2}
    assert stepped(lambda g: optim.FusedAdam(g, lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)) == \
        {"zsv_grad_norm_multi": 2, "zsv_grad_norm_finalize": 1, "zsv_adamw_multi": 2}
    assert stepped(lambda g: optim.FusedSGD(g, lr=0.1, momentum=0.9)) == {"zsv_sgd_multi": 2}
    assert stepped(lambda g: optim.FusedSGD(g, lr=0.1, momentum=0.9, max_grad_norm=1.0)) == \
        {"zsv_grad_norm_multi": 2, "zsv_grad_norm_finalize": 1, "zsv_sgd_multi": 2}
    assert stepped(lambda g: optim.FusedLARS(g, lr=0.1)) == {"zsv_lars_norms": 2, "zsv_layerwise_finalize": 2, "zsv_lars_multi": 2}
    assert stepped(lambda g: optim.FusedLAMB(g)) == {"zsv_lamb_moments": 2, "zsv_layerwise_finalize": 2, "zsv_lamb_multi": 2}
