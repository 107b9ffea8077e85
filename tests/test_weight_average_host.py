"""Weight averaging without a device: the C ABI is declared and bound, ``optim.WeightAverage`` refuses bad arguments before it
touches a device, and ``train.load_weights(key=)`` reads the averaged state dict of a checkpoint."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ["zsv_adam_multi_avg", "zsv_adam_multi_scaled_avg", "zsv_adamw_multi_avg", "zsv_adamw_multi_scaled_avg", "zsv_avg_multi",
       "zsv_avg_advance", "zsv_swap_multi"]


def test_averaging_entry_points_are_declared_exported_and_bound():
    from zeroshotvideoclassification_amd import _lib
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    declared = set(re.findall(r"\b(zsv_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and "zsv_avg_state" in header and "zsv_pair_tensor" in header
    assert declared == set(_lib.SIGNATURES)
    lib = _lib.load()                                       # AttributeError if a symbol is not exported
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    P, i32, i64, f32, f64 = _lib._P, _lib.c_int32, _lib.c_int64, _lib.c_float, _lib.c_double
    tail = [P, P, f32, P]                                   # shadows, averaging state, ema_weight, stream
    # each *_avg form is its plain form with the averaging arguments in front of the stream
    for plain in ("zsv_adam_multi", "zsv_adam_multi_scaled", "zsv_adamw_multi", "zsv_adamw_multi_scaled"):
        assert _lib.SIGNATURES[plain + "_avg"][1] == _lib.SIGNATURES[plain][1][:-1] + tail, plain
    assert _lib.SIGNATURES["zsv_avg_multi"][1] == [P, i32, i64, P, f32, P, P]
    assert _lib.SIGNATURES["zsv_avg_advance"][1] == [P, P, P]
    assert _lib.SIGNATURES["zsv_swap_multi"][1] == [P, i32, i64, P]
    # the existing entry points keep their signatures
    assert _lib.SIGNATURES["zsv_adam_multi"][1] == [P, i32, i64, f32, f32, f32, f32, i32, P]
    assert _lib.SIGNATURES["zsv_adamw_multi_scaled"][1] == [P, i32, i64, f64, f32, f32, f32, f64, i32, P, P, i32, P]


def test_constructor_checks_need_no_device():
    from zeroshotvideoclassification_amd import optim
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(TypeError, match="FusedAdam"):
        optim.WeightAverage(torch.optim.Adam(ps, lr=1e-3))
    with pytest.raises(TypeError, match="FusedAdam"):
        optim.WeightAverage(None)
    opt = optim.FusedAdam(ps, lr=1e-3)
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", True):
        with pytest.raises(ValueError, match="decay"):
            optim.WeightAverage(opt, decay=bad)
    assert opt._average is None                             # a refused construction leaves the optimizer as it was


def _checkpoint(path, with_average):
    from zeroshotvideoclassification_amd import train
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    live = {train._PREFIX + k: v.detach().clone() for k, v in model.state_dict().items()}
    ckpt = {"state_dict": live, "opt": None, "accuracy": 0.5}
    if with_average:
        ckpt["state_dict_avg"] = {k: (v + 1 if v.is_floating_point() else v.clone()) for k, v in live.items()}
    torch.save(ckpt, path)
    return model, live


def test_load_weights_reads_the_averaged_state_dict(tmp_path):
    from zeroshotvideoclassification_amd import train
    path = str(tmp_path / "ckpt.pth.tar")
    model, live = _checkpoint(path, with_average=True)
    fresh = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    assert train.load_weights(fresh, path, key="state_dict_avg") == len(live)
    for k, v in fresh.state_dict().items():
        want = live[train._PREFIX + k]
        assert torch.equal(v, want + 1 if v.is_floating_point() else want), k
    assert train.load_weights(fresh, path) == len(live)     # the default is still "state_dict"
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, live[train._PREFIX + k]), k


def test_a_missing_key_names_the_keys_the_file_has(tmp_path):
    from zeroshotvideoclassification_amd import train
    path = str(tmp_path / "plain.pth.tar")
    model, _ = _checkpoint(path, with_average=False)
    with pytest.raises(KeyError) as info:
        train.load_weights(model, path, key="state_dict_avg")
    message = str(info.value)
    assert "state_dict_avg" in message
    for key in ("accuracy", "opt", "'state_dict'"):
        assert key in message, message
