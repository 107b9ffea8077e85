"""Which kernel serves a weight gradient, in how many slices and with how much workspace, without a GPU: the size queries and
the refusals of ``zsv_conv3d_wgrad*`` are decided on the host and return before anything is launched or dereferenced.  The rows
and switch sets are in ``wgrad_cases.py``; the answers were recorded by ``tools/make_wgrad_host_golden.py`` and pin the route
table and the slice arithmetic of every plan (csrc/conv_wgrad.hip, csrc/wgrad_plan.h).
"""
import json
import os

import pytest

import wgrad_cases as W
import test_ops_gpu as T
from zeroshotvideoclassification_amd import _lib, ops

ROWS = W.rows(T.WGRAD_DMA_CASES, T.WGRAD_WINO_CASES, T.WGRAD_TRING_CASES)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "wgrad_host_answers.json")) as f:
        return json.load(f)


def test_the_recording_covers_exactly_the_rows_and_switch_sets(recorded):
    assert sorted(recorded) == sorted(f"{r.name} {W.switch_id(s)}" for r in ROWS for s in W.SWITCH_SETS)
    # (the rows do reach every route: some take the tap-validity table, some the prologue, some need no workspace at all)
    assert {a["mask_bytes"] > 0 for a in recorded.values()} == {True, False}
    assert {a["pre_supported"] for a in recorded.values()} == {0, 1}
    assert len({a["workspace_bytes"] for a in recorded.values()}) > 100


@pytest.mark.parametrize("switches", W.SWITCH_SETS, ids=[W.switch_id(s) for s in W.SWITCH_SETS])
def test_every_row_gives_the_recorded_answers(switches, recorded, monkeypatch):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    lib = _lib.load()
    wrong = []
    for row in ROWS:
        got = W.answers(lib, ops.conv_desc(row.xs, row.ws, row.stride, row.padding))
        want = recorded[f"{row.name} {W.switch_id(switches)}"]
        if got != want:
            wrong.append((row.name, {k: (got[k], want[k]) for k in want if got.get(k) != want[k]}))
    assert not wrong, wrong
