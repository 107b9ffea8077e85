"""Generate ``tests/golden/*.npz`` from the REFERENCE's own modules -- TEST INFRASTRUCTURE.

Run in the build container only (needs ``/root/reference``):

    python -m oracle.make_golden

For each case the reference model (``network.get_network`` imported through
``oracle/reference_import.py``) is given the name-keyed synthetic weights and the
synthetic clips of ``zeroshotvideoclassification_amd.synthetic``; inputs are
regenerated from seeds on the consuming side, so only the expected outputs are stored.
Every case also checks that ``oracle/restatement.py`` reproduces the reference
bit-for-bit on the same inputs (the restatement is what travels to the GPU box).
"""
from __future__ import annotations

import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import restatement as R                                   # noqa: E402
from oracle.reference_import import (import_reference, import_reference_transforms,    # noqa: E402
                                     reference_main_functions)
from oracle import transforms_oracle as TO                              # noqa: E402
from zeroshotvideoclassification_amd import synthetic as S             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# name, network, N, T, HW, bn_jitter, train?
CASES = [
    dict(name="r2plus1d_A", network="r2plus1d_18", n=2, frames=16, size=112, bn_jitter=False),
    dict(name="r2plus1d_jitter", network="r2plus1d_18", n=2, frames=16, size=112, bn_jitter=True),
    dict(name="r2plus1d_small", network="r2plus1d_18", n=3, frames=8, size=56, bn_jitter=True),
    dict(name="r3d_small", network="r3d_18", n=2, frames=8, size=56, bn_jitter=True),
    dict(name="c3d_eval", network="c3d", n=1, frames=16, size=112, bn_jitter=False),
]


def sample_idx(numel: int, k: int = 64) -> np.ndarray:
    return np.unique(np.linspace(0, numel - 1, num=min(k, numel)).astype(np.int64))


def bn_inputs_stats(model):
    """Hook every BatchNorm3d: batch mean / biased var of its input, in call order."""
    stats, hooks = OrderedDict(), []
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            def hook(mod, inp, _out, name=name):
                x = inp[0].detach().double()
                stats[name] = (x.mean(dim=(0, 2, 3, 4)).float().numpy(),
                               x.var(dim=(0, 2, 3, 4), unbiased=False).float().numpy())
            hooks.append(m.register_forward_hook(hook))
    return stats, hooks


def run_case(case, ref_network):
    opt = R.make_opt(case["network"])
    torch.manual_seed(0)
    ref = ref_network.get_network(opt)
    mine = R.oracle_network(opt)
    sd_ref = ref.state_dict()
    sd_mine = mine.state_dict()
    assert list(sd_ref.keys()) == list(sd_mine.keys()), "state_dict keys/order differ from the reference"
    for k in sd_ref:
        assert sd_ref[k].shape == sd_mine[k].shape, k
    weights = S.keyed_state_dict(sd_ref, seed=0, bn_jitter=case["bn_jitter"])
    ref.load_state_dict(weights)
    mine.load_state_dict(weights)

    n = case["n"]
    x = S.synthetic_clips(n, case["frames"], case["size"])
    _, z = S.synthetic_targets(n)
    out = {}
    is_c3d = case["network"] == "c3d"
    if is_c3d:          # dropout makes train mode RNG dependent: eval parity
        ref.eval(); mine.eval()
    else:
        ref.train(); mine.train()

    # ---- fp32 forward + backward on the reference; restatement must match bit for bit
    stats, hooks = ({}, [])
    if not is_c3d:
        stats, hooks = bn_inputs_stats(ref)
    y_ref = R.embed(ref, x)
    loss_ref = F.mse_loss(y_ref, z)
    loss_ref.backward()
    for h in hooks:
        h.remove()
    y_mine = R.embed(mine, x)
    loss_mine = F.mse_loss(y_mine, z)
    loss_mine.backward()
    assert torch.equal(y_ref, y_mine), "restatement forward differs from the reference"
    assert torch.equal(loss_ref, loss_mine)
    g_ref = {k: p.grad for k, p in ref.named_parameters()}
    g_mine = {k: p.grad for k, p in mine.named_parameters()}
    for k in g_ref:
        assert (g_ref[k] is None) == (g_mine[k] is None), k
        if g_ref[k] is not None:
            assert torch.equal(g_ref[k], g_mine[k]), f"restatement grad differs: {k}"
    out["emb_f32"] = y_ref.detach().numpy()
    out["loss_f32"] = np.float64(loss_ref.item())
    out["live_params"] = np.array([k for k, g in g_ref.items() if g is not None])
    out["dead_params"] = np.array([k for k, g in g_ref.items() if g is None])
    if stats:
        out["bn_names"] = np.array(list(stats.keys()))
        out["bn_mean"] = np.concatenate([v[0] for v in stats.values()])
        out["bn_var"] = np.concatenate([v[1] for v in stats.values()])

    # stage statistics (trunk models only)
    if not is_c3d:
        with torch.no_grad():
            trunk = ref.model
            t = x.reshape(n, *x.shape[2:])
            feats = [trunk.stem(t)]
            for i in range(1, 5):
                feats.append(getattr(trunk, f"layer{i}")(feats[-1]))
        for name, f in zip(["stem", "layer1", "layer2", "layer3", "layer4"], feats):
            flat = f.flatten()
            out[f"stage_{name}_mean"] = np.float64(flat.double().mean().item())
            out[f"stage_{name}_absmean"] = np.float64(flat.double().abs().mean().item())
            out[f"stage_{name}_sample"] = flat[sample_idx(flat.numel())].numpy()
        # NOTE: the no_grad forward above ran BN in train mode once more -> running stats were
        # updated twice so far on ``ref``; the step below re-loads weights to keep this clean.

    # ---- fp64 reference: embeddings, loss, per-parameter gradient norms + samples
    ref64 = ref_network.get_network(opt).double()
    ref64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in weights.items()})
    ref64.eval() if is_c3d else ref64.train()
    y64 = R.embed(ref64, x.double())
    loss64 = F.mse_loss(y64, z.double())
    loss64.backward()
    out["emb_f64"] = y64.detach().numpy()
    out["loss_f64"] = np.float64(loss64.item())
    names, norms, samples = [], [], []
    for k, p in ref64.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.flatten()
        names.append(k)
        norms.append(g.norm().item())
        s = np.zeros(16)
        idx = sample_idx(g.numel(), 16)
        s[:len(idx)] = g[idx].numpy()
        samples.append(s)
    out["grad_names"] = np.array(names)
    out["grad_norm_f64"] = np.array(norms)
    out["grad_sample_f64"] = np.stack(samples)

    # ---- one full Adam step in fp32 from fresh weights, then eval-mode embeddings
    if not is_c3d:
        ref.load_state_dict(weights)
        ref.train()
        opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
        y1, l1 = R.train_step(ref, opt_ref, x, z)
        sd_after = ref.state_dict()
        rm = [sd_after[k].numpy() for k in sd_after if k.endswith("running_mean")]
        rv = [sd_after[k].numpy() for k in sd_after if k.endswith("running_var")]
        out["running_mean_after1"] = np.concatenate(rm)
        out["running_var_after1"] = np.concatenate(rv)
        out["step1_loss"] = np.float64(l1.item())
        y2, l2 = R.train_step(ref, opt_ref, x, z)
        out["step2_loss"] = np.float64(l2.item())
        # eval-mode embeddings from the *initial* weights (deterministic, no Adam sign noise)
        ref.load_state_dict(weights)
        ref.eval()
        with torch.no_grad():
            out["emb_eval_f32"] = R.embed(ref, x).numpy()
            if case["name"] == "r2plus1d_jitter":      # config E shape: 32-frame clips, eval BN
                x32 = S.synthetic_clips(1, 32, case["size"], seed=99)
                out["emb_eval_t32_f32"] = R.embed(ref, x32).numpy()
    else:
        ref.eval()
        with torch.no_grad():
            out["emb_eval_f32"] = R.embed(ref, x).numpy()
    return out


# ---------------------------------------------------------------------------------------------
# clip transforms: outputs of the reference's own ``get_transform`` chains
TRANSFORM_SIZES = [(120, 160), (240, 320), (128, 171), (200, 130)]


def transform_input(h: int, w: int, frames: int = 1) -> torch.Tensor:
    """The uint8 ``(T, H, W, 3)`` clip of a transforms case (regenerated by the tests)."""
    g = torch.Generator().manual_seed(h * 1000 + w)
    return torch.randint(0, 256, (frames, h, w, 3), dtype=torch.uint8, generator=g)


def run_transforms():
    """``get_transform(True)`` / ``get_transform(False)`` (transforms.py:41-56) of the reference on seeded
    uint8 clips.  The training chain draws its crop / flip from Python's ``random``: the draws are
    replayed through ``preprocess.ClipTransform.draw_params`` (same seed) and must reproduce the
    reference's output through the restatement bit for bit -- that pins the draw order too."""
    import random
    from zeroshotvideoclassification_amd import preprocess
    RT = import_reference_transforms()
    out = {"sizes": np.array(TRANSFORM_SIZES)}
    for k, (h, w) in enumerate(TRANSFORM_SIZES):
        clip = transform_input(h, w)
        hres, wres, _ = preprocess.resized_hw(h, w, 128)
        val = RT.get_transform(True)(clip)
        assert tuple(val.shape) == (3, 1, 112, 112)
        ci, cj = TO.center_crop_params(hres, wres, 112, 112)
        assert torch.equal(val, TO.clip_transform(clip, ci, cj, False)), "restatement differs (validation chain)"
        out[f"val_{h}x{w}"] = val.numpy()
        seed = 100 + k
        random.seed(seed)
        trn = RT.get_transform(False)(clip)
        random.seed(seed)
        (i, j, f), = preprocess.ClipTransform(False).draw_params(1, hres, wres)
        assert torch.equal(trn, TO.clip_transform(clip, i, j, bool(f))), "restatement / draw order differs (training chain)"
        out[f"train_{h}x{w}"] = trn.numpy()
        out[f"train_params_{h}x{w}"] = np.array([seed, i, j, f])
    return out


# multi-frame clips (the single-frame fixtures above cannot see a frame-index error): one validation and one training case
TRANSFORM_T4 = [("val", 120, 160, 4), ("train", 200, 130, 4)]


def run_transforms_t4():
    """The same two chains of the reference on 4-frame clips (``tests/golden/transforms_t4.npz``)."""
    import random
    from zeroshotvideoclassification_amd import preprocess
    RT = import_reference_transforms()
    out = {"cases": np.array([f"{kind}_{h}x{w}x{t}" for kind, h, w, t in TRANSFORM_T4])}
    for k, (kind, h, w, t) in enumerate(TRANSFORM_T4):
        clip = transform_input(h, w, t)
        hres, wres, _ = preprocess.resized_hw(h, w, 128)
        if kind == "val":
            got = RT.get_transform(True)(clip)
            ci, cj = TO.center_crop_params(hres, wres, 112, 112)
            assert torch.equal(got, TO.clip_transform(clip, ci, cj, False)), "restatement differs (validation chain, T=4)"
            params = [0, ci, cj, 0]
        else:
            seed = 200 + k
            random.seed(seed)
            got = RT.get_transform(False)(clip)
            random.seed(seed)
            (i, j, f), = preprocess.ClipTransform(False).draw_params(1, hres, wres)
            assert torch.equal(got, TO.clip_transform(clip, i, j, bool(f))), "restatement / draw order differs (training chain, T=4)"
            params = [seed, i, j, f]
        assert tuple(got.shape) == (3, t, 112, 112)
        assert not torch.equal(got[:, 0], got[:, 1])                      # frames differ: an index mix-up would show
        out[f"{kind}_{h}x{w}x{t}"] = got.numpy()
        out[f"{kind}_params_{h}x{w}x{t}"] = np.array(params)
    return out


# ---------------------------------------------------------------------------------------------
# evaluate() / compute_accuracy(): the reference's own functions on synthetic embeddings
EVAL_SETS = [dict(name="ucf101", classes=101, n=1500), dict(name="hmdb51", classes=51, n=900),
             dict(name="activitynet", classes=200, n=2000)]


def run_accuracy():
    """``evaluate`` (main.py:224-313) and ``compute_accuracy`` (main.py:316-325) compiled from the
    reference's text (``reference_main_functions``) and run with stand-ins for their globals: the
    "model" returns its input (the batches carry the predicted embeddings), the loader yields
    ``(X, l, Z, _)`` batches with some broken samples (label -1), ``opt.split == -1`` selects the
    10-split protocol, and the tensorboard writer records the scalars."""
    import tempfile
    from types import SimpleNamespace
    from scipy.spatial.distance import cdist
    from sklearn.metrics import accuracy_score
    out = {}
    for spec in EVAL_SETS:
        table, labels, true, pred = S.synthetic_eval_set(spec["n"], spec["classes"], broken=7)
        scalars = {}
        writer = SimpleNamespace(add_scalar=lambda tag, v, epoch: scalars.__setitem__(tag, float(v)))
        dataset = SimpleNamespace(name=spec["name"], class_embed=table.numpy())
        dataset_len = spec["n"]

        class Loader:
            def __init__(self):
                self.dataset = type("D", (), {"name": dataset.name, "class_embed": dataset.class_embed,
                                              "__len__": lambda self_: dataset_len})()

            def __iter__(self):
                for a in range(0, spec["n"], 64):
                    yield pred[a:a + 64], labels[a:a + 64], true[a:a + 64], None

        with tempfile.TemporaryDirectory() as tmp:
            opt = SimpleNamespace(dataset="synthetic", progressbar=False, device="cpu", savename=tmp, split=-1)
            ns = reference_main_functions(
                model=torch.nn.Identity(), opt=opt, np=np, torch=torch, cdist=cdist, accuracy_score=accuracy_score,
                tqdm=lambda it, **_k: it, Fore=SimpleNamespace(RED="", GREEN=""), Style=SimpleNamespace(RESET_ALL=""))
            acc, acc5 = ns["evaluate"](Loader(), writer, 0)
        keep = labels != -1
        mine = R.evaluate_protocol(pred[keep].numpy(), true[keep].numpy(), labels[keep].numpy(), table.numpy())
        name = spec["name"]
        got = {"accuracy": acc, "accuracy_top5": acc5, "split_accuracy": scalars[name + "/AccSplit_Mean"],
               "split_accuracy_std": scalars[name + "/AccSplit_Std"],
               "split_accuracy_top5": scalars[name + "/AccSplit_Mean_Top5"],
               "split_accuracy_top5_std": scalars[name + "/AccSplit_Std_Top5"]}
        assert scalars[name + "/Accuracy"] == acc and scalars[name + "/Accuracy_Top5"] == acc5
        for k, v in got.items():
            assert mine[k] == v, f"restatement of evaluate differs from the reference: {name} {k} {mine[k]} {v}"
        direct = ns["compute_accuracy"](pred[keep].numpy(), table.numpy(), true[keep].numpy())
        assert tuple(direct) == (acc, acc5)
        out[name + "_spec"] = np.array([spec["classes"], spec["n"], 7])
        out[name + "_expected"] = np.array([got[k] for k in sorted(got)])
        out[name + "_keys"] = np.array(sorted(got))
        out[name + "_n_kept"] = np.array(int(keep.sum()))
        print(f"  {name}: " + ", ".join(f"{k}={v:.4f}" for k, v in got.items()), flush=True)
    return out


# ---------------------------------------------------------------------------------------------
# module surface that no factory / get_network reaches: Bottleneck (resnet.py:116-162), ResNet18 head (network.py:50-80)
def run_surface_extras():
    """The reference's own ``Bottleneck`` blocks inside ``VideoResNet`` (one per stage, (2+1)D convolutions) and the
    original ``ResNet18`` single-Linear head, on name-keyed weights and seeded clips: forward (train-mode BatchNorm for the
    trunk; eval for the head, whose dropout is RNG-dependent) + the fp64 gradient norms of every parameter."""
    ref_network, ref_resnet = import_reference()
    out = {}
    x = S.synthetic_clips(2, 4, 32, seed=21)

    def grads64(build, run, mode_train):
        m = build().double()
        if hasattr(m, "dropout"):
            m.dropout = torch.nn.Identity()                  # (train-mode gradients without the RNG-dependent mask)
        m.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in weights.items()})
        m.train(mode_train)
        y = run(m, x.double())
        # (an L2-normalised head makes sum(y^2) constant: project on the synthetic targets instead)
        ((y * S.synthetic_targets(2)[1].double()).sum() if y.shape[1] == 300 else (y * y).sum()).backward()
        names = [k for k, p in m.named_parameters() if p.grad is not None]
        return y.detach().numpy(), np.array(names), np.array([dict(m.named_parameters())[k].grad.norm().item() for k in names])

    def bottleneck_trunk():
        return ref_resnet.VideoResNet(block=ref_resnet.Bottleneck, conv_makers=[ref_resnet.Conv2Plus1D] * 4, layers=[1, 1, 1, 1],
                                      stem=ref_resnet.R2Plus1dStem)
    torch.manual_seed(0)
    m = bottleneck_trunk()
    weights = S.keyed_state_dict(m.state_dict(), seed=3, bn_jitter=True)
    m.load_state_dict(weights)
    m.train()
    pooled, f = m(x.reshape(2, 3, 4, 32, 32))
    out["bottleneck_keys"] = np.array(list(m.state_dict().keys()))
    out["bottleneck_pooled_f32"] = pooled.detach().numpy()
    out["bottleneck_feature_shape"] = np.array(f.shape)
    y64, names, norms = grads64(bottleneck_trunk, lambda mod, xx: mod(xx.reshape(2, 3, 4, 32, 32))[0], True)
    out["bottleneck_pooled_f64"], out["bottleneck_grad_names"], out["bottleneck_grad_norm_f64"] = y64, names, norms

    def head():
        return ref_network.ResNet18(ref_resnet.r2plus1d_18, fixconvs=False, nopretrained=False)
    m = head()
    weights = S.keyed_state_dict(m.state_dict(), seed=4, bn_jitter=True)
    m.load_state_dict(weights)
    m.eval()
    with torch.no_grad():
        out["resnet18_emb_eval_f32"] = m(x).numpy()
    out["resnet18_keys"] = np.array(list(m.state_dict().keys()))
    y64, names, norms = grads64(head, lambda mod, xx: mod(xx), True)
    out["resnet18_emb_train_nodrop_f64"], out["resnet18_grad_names"], out["resnet18_grad_norm_f64"] = y64, names, norms
    return out


# ---------------------------------------------------------------------------------------------
# config E at batch size > 1: 32-frame eval embeddings of the reference for FOUR clips (the per-case fixture holds one)
def run_t32_batch():
    """``emb_eval_t32_f32``: R(2+1)D-18 ``Model`` in eval mode (jittered BatchNorm statistics) on 4 clips of 32 frames at
    112x112, from the imported reference; the bf16 engine and the folded fp32 engine are checked against it."""
    ref_network, _ = import_reference()
    opt = R.make_opt("r2plus1d_18")
    ref = ref_network.get_network(opt)
    mine = R.oracle_network(opt)
    weights = S.keyed_state_dict(ref.state_dict(), seed=0, bn_jitter=True)
    ref.load_state_dict(weights)
    mine.load_state_dict(weights)
    ref.eval(); mine.eval()
    x = S.synthetic_clips(4, 32, 112, seed=199)
    with torch.no_grad():
        y = R.embed(ref, x)
        assert torch.equal(y, R.embed(mine, x)), "restatement differs from the reference (T=32 eval, N=4)"
    return {"emb_eval_t32_f32": y.numpy(), "meta_n": np.array(4), "meta_frames": np.array(32), "meta_size": np.array(112),
            "meta_seed": np.array(199), "meta_bn_jitter": np.array(True), "meta_network": np.array("r2plus1d_18")}


# ---------------------------------------------------------------------------------------------
# the reference's mixed-precision step (main.py:172 `with autocast():`, main.py:137,195-203 GradScaler) in bf16
AUTOCAST_CASE = dict(network="r2plus1d_18", n=3, frames=8, size=56, bn_jitter=True, steps=30, lr=1e-3)


def run_autocast_bf16():
    """The imported reference under ``torch.autocast("cpu", dtype=torch.bfloat16)`` -- main.py:170-203's forward and loss
    inside the context, backward outside -- on the ``r2plus1d_small`` inputs: embeddings, loss, per-parameter gradient norms
    and samples of the first step, BatchNorm running statistics after it, and the loss of 30 Adam steps (with the fp32
    curve of the same steps next to it).  ``amp.autocast`` + ``amp`` training path are checked against these."""
    c = AUTOCAST_CASE
    ref_network, _ = import_reference()
    opt = R.make_opt(c["network"])
    torch.manual_seed(0)
    ref = ref_network.get_network(opt)
    weights = S.keyed_state_dict(ref.state_dict(), seed=0, bn_jitter=c["bn_jitter"])
    x = S.synthetic_clips(c["n"], c["frames"], c["size"])
    _, z = S.synthetic_targets(c["n"])
    out = {}

    def step(model, optim, autocast):
        optim.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            y = R.embed(model, x)
            loss = F.mse_loss(y, z)                      # (autocast runs mse_loss in fp32)
        loss.backward()
        optim.step()
        return y, loss

    ref.load_state_dict(weights)
    ref.train()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = R.embed(ref, x)
        loss = F.mse_loss(y, z)
    loss.backward()
    out["emb"] = y.detach().float().numpy()
    out["emb_dtype"] = np.array(str(y.dtype))
    out["loss"] = np.float64(loss.item())
    names, norms, samples = [], [], []
    for k, p in ref.named_parameters():
        if p.grad is None:
            continue
        assert p.grad.dtype == torch.float32, k        # parameters and their gradients stay fp32 under autocast
        g = p.grad.flatten()
        names.append(k)
        norms.append(g.double().norm().item())
        smp = np.zeros(16)
        idx = sample_idx(g.numel(), 16)
        smp[:len(idx)] = g[idx].numpy()
        samples.append(smp)
    out["grad_names"], out["grad_norm"], out["grad_sample"] = np.array(names), np.array(norms), np.stack(samples)
    sd = ref.state_dict()
    grads16 = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
    out["running_mean_after1"] = np.concatenate([sd[k].numpy() for k in sd if k.endswith("running_mean")])
    out["running_var_after1"] = np.concatenate([sd[k].numpy() for k in sd if k.endswith("running_var")])
    # how far the reference's OWN bf16 gradients are from its fp32 gradients on this problem (random-init weights, a loss
    # gradient that is tiny next to bf16's rounding of the activations): the noise floor the HIP path is held to
    ref.load_state_dict(weights)
    ref.train()
    ref.zero_grad()
    F.mse_loss(R.embed(ref, x), z).backward()
    cosines = []
    for k in names:
        a, b = grads16[k].double().flatten(), dict(ref.named_parameters())[k].grad.double().flatten()
        cosines.append(float(a @ b / (a.norm() * b.norm() + 1e-300)))
    out["grad_cos_vs_f32"] = np.array(cosines)
    out["grad_norm_f32"] = np.array([dict(ref.named_parameters())[k].grad.double().norm().item() for k in names])
    for tag, autocast in (("bf16", True), ("f32", False)):
        ref.load_state_dict(weights)
        ref.train()
        optim = torch.optim.Adam(ref.parameters(), lr=c["lr"])
        out[f"loss_curve_{tag}"] = np.array([step(ref, optim, autocast)[1].item() for _ in range(c["steps"])])
    for k, v in c.items():
        out["meta_" + k] = np.array(v)
    return out


def run_autocast_bf16_c3d():
    """The imported reference's C3D (network.py:95-180) under ``torch.autocast("cpu", dtype=torch.bfloat16)``, eval mode (its
    dropout is RNG-dependent; C3D has no BatchNorm, so eval == train otherwise), one 16x112x112 clip: embedding, loss, and
    per-parameter gradient norms / cosines against its own fp32 gradients -- the noise floor ``amp.Bf16TrainPathC3D`` is held to."""
    ref_network, _ = import_reference()
    opt = R.make_opt("c3d")
    torch.manual_seed(0)
    ref = ref_network.get_network(opt)
    weights = S.keyed_state_dict(ref.state_dict(), seed=0, bn_jitter=False)
    ref.load_state_dict(weights)
    ref.eval()
    x = S.synthetic_clips(1, 16, 112)
    _, z = S.synthetic_targets(1)
    out = {}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y = R.embed(ref, x)
        loss = F.mse_loss(y, z)
    loss.backward()
    out["emb"] = y.detach().float().numpy()
    out["loss"] = np.float64(loss.item())
    names = [k for k, p in ref.named_parameters() if p.grad is not None]
    g16 = {k: dict(ref.named_parameters())[k].grad.detach().clone() for k in names}
    ref.zero_grad()
    y32 = R.embed(ref, x)
    loss32 = F.mse_loss(y32, z)
    loss32.backward()
    g32 = {k: dict(ref.named_parameters())[k].grad.detach().clone() for k in names}
    out["emb_f32"] = y32.detach().numpy()
    out["loss_f32"] = np.float64(loss32.item())
    out["grad_names"] = np.array(names)
    out["grad_norm"] = np.array([g16[k].double().norm().item() for k in names])
    out["grad_norm_f32"] = np.array([g32[k].double().norm().item() for k in names])
    cos = []
    for k in names:
        a, b = g16[k].double().flatten(), g32[k].double().flatten()
        cos.append(float(a @ b / (a.norm() * b.norm() + 1e-300)))
    out["grad_cos_vs_f32"] = np.array(cos)
    out["meta_n"], out["meta_frames"], out["meta_size"], out["meta_network"] = np.array(1), np.array(16), np.array(112), np.array("c3d")
    return out


PIN_NETWORKS = ("r2plus1d_18", "r3d_18", "c3d")


def pin_case(name: str):
    """Inputs of ``tests/test_oracle.py::test_restatement_is_pinned_to_the_imported_reference`` for one network: keyed weights
    (seed 5, BatchNorm jitter), clips (seed 8), train mode except C3D (eval)."""
    size, frames, n = (112, 16, 1) if name == "c3d" else (32, 4, 2)
    return dict(weights_seed=5, clip_seed=8, n=n, frames=frames, size=size, train=name != "c3d")


def run_restatement_pin():
    """``restatement_pin.npz``: what the REFERENCE's networks compute on the pinning test's inputs -- the ``state_dict`` keys,
    the embeddings, which parameters get no gradient, and per live parameter the fp64 norm of its gradient and its values at
    ``sample_idx`` -- after checking that the restatement reproduces the reference bit for bit on the same inputs."""
    ref_network, _ = import_reference()
    out = {}
    for name in PIN_NETWORKS:
        c = pin_case(name)
        opt = R.make_opt(name)
        ref, mine = ref_network.get_network(opt), R.oracle_network(opt)
        assert list(ref.state_dict().keys()) == list(mine.state_dict().keys()), name
        weights = S.keyed_state_dict(ref.state_dict(), seed=c["weights_seed"], bn_jitter=True)
        ref.load_state_dict(weights)
        mine.load_state_dict(weights)
        x = S.synthetic_clips(c["n"], c["frames"], c["size"], seed=c["clip_seed"])
        for m in (ref, mine):
            m.train(c["train"])
        ya, yb = R.embed(ref, x), R.embed(mine, x)
        assert torch.equal(ya, yb), name
        ya.sum().backward()
        yb.sum().backward()
        names, norms, samples = [], [], []
        for (k, p), (_, q) in zip(ref.named_parameters(), mine.named_parameters()):
            assert (p.grad is None) == (q.grad is None), k
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), k
                g = p.grad.detach().reshape(-1)
                names.append(k)
                norms.append(g.double().norm().item())
                samples.append(g[torch.from_numpy(sample_idx(g.numel()))].numpy())
        out[f"{name}_state_keys"] = np.array(list(ref.state_dict().keys()))
        out[f"{name}_emb_f32"] = ya.detach().numpy()
        out[f"{name}_dead_params"] = np.array([k for k, p in ref.named_parameters() if p.grad is None], dtype=str)
        out[f"{name}_grad_names"] = np.array(names)
        out[f"{name}_grad_norm_f64"] = np.array(norms, dtype=np.float64)
        out[f"{name}_grad_sample_f32"] = np.concatenate(samples).astype(np.float32)
        out.update({f"{name}_meta_{k}": np.array(v) for k, v in c.items()})
    return out


def main():
    torch.set_num_threads(os.cpu_count() or 8)
    ref_network, _ = import_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    only = set(sys.argv[1:])
    for name, fn in (("transforms", run_transforms), ("transforms_t4", run_transforms_t4), ("accuracy", run_accuracy),
                     ("surface_extras", run_surface_extras), ("r2plus1d_t32_batch", run_t32_batch),
                     ("r2plus1d_small_autocast_bf16", run_autocast_bf16), ("c3d_autocast_bf16", run_autocast_bf16_c3d),
                     ("restatement_pin", run_restatement_pin)):
        if only and name not in only:
            continue
        t0 = time.time()
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **fn(), meta_torch=np.array(torch.__version__))
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB in {time.time() - t0:.1f}s", flush=True)
    for case in CASES:
        if only and case["name"] not in only:
            continue
        t0 = time.time()
        out = run_case(case, ref_network)
        meta = {"meta_" + k: np.array(v) for k, v in case.items()}
        meta["meta_torch"] = np.array(torch.__version__)
        path = os.path.join(GOLDEN, case["name"] + ".npz")
        np.savez_compressed(path, **out, **meta)
        print(f"{case['name']}: {os.path.getsize(path) / 1024:.1f} KiB in {time.time() - t0:.1f}s "
              f"loss32={out['loss_f32']:.8f} loss64={out['loss_f64']:.8f}", flush=True)


if __name__ == "__main__":
    main()
