"""Frozen-BatchNorm surface that needs no GPU: evaluate() keeps per-module modes, the new entry points are declared and bound."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import make_opt  # noqa: E402
from zeroshotvideoclassification_amd import _lib, network, torch_ops, train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evaluate_restores_each_modules_own_mode(monkeypatch):
    """A training-mode model whose stem and layer1 BatchNorms are frozen comes back from evaluate() exactly as it went in
    (model.train(True) would have switched the frozen BatchNorms back to batch statistics)."""
    model = network.get_network(make_opt("r2plus1d_18"))
    model.train()
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm3d) and name.startswith(("model.stem", "model.layer1")):
            m.eval()
    before = {name: m.training for name, m in model.named_modules()}
    assert not all(before.values()) and any(before.values())
    seen = []

    def fake_embed(forward, x):
        seen.append({name: m.training for name, m in model.named_modules()})
        return torch.nn.functional.normalize(torch.ones(x.shape[0], 300), dim=1)

    monkeypatch.setattr(train, "embed", fake_embed)
    monkeypatch.setattr(train, "compute_accuracy", lambda pred, classes, true: (0.0, 0.0))     # (the scoring runs on the device)
    x = torch.zeros(2, 1, 3, 4, 8, 8)
    batches = [(x, torch.tensor([0, 1]), torch.randn(2, 300))]
    out = train.evaluate(model, batches, torch.randn(4, 300), device=torch.device("cpu"), splits=0)
    assert out["n"] == 2
    assert seen and not any(seen[0].values())                     # everything in eval mode during the evaluation
    assert {name: m.training for name, m in model.named_modules()} == before


def test_frozen_batchnorm_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    for sym in ("zsv_bn_bwd_eval", "zsv_bn_eval_coeffs", "zsv_bn_cl_fwd_eval", "zsv_bn_cl_bwd_eval"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    for op in ("bn_eval_fwd", "bn_eval_bwd", "batch_norm_relu_eval"):
        assert op in torch_ops.OPERATORS
