"""Host half of the Winograd instantiation matrix (tests/wino_cases.py): no GPU, needs the built library.

* the preconditions of every launch of the matrix, in both operand kinds;
* every switch the matrix sets is a name in ZSV_KNOB_LIST;
* under every (case, switches) the restated planners give the library's own answers (workspace bytes, statistics tiles, the three
  "supported" queries; the queries dereference nothing);
* the expected instantiations over the whole matrix are all 46, so a retune that moves a case off its kernel fails here;
* the fp64 restatement of the Winograd algorithm is the convolution, and its absolute-value form dominates it.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import wino_cases as W
from zeroshotvideoclassification_amd import _lib, ops

ALIGNED_DUMMY = 0x1000      # a 16-byte aligned address for the statistics-tile query, never dereferenced
RUNS = W.runs()


def _desc(g):
    return ops.conv_desc(g.xs, (g.cout, g.xs[1]) + g.kernel, g.stride, g.padding)


def _setenv(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def test_row_tiling():
    """47: one ragged 48-row tile; 65: two, 17 live rows in the second; 63: one ragged 64-row tile; 97: two, 33 live rows."""
    assert [W.wino_tm(m) for m in (47, 65, 63, 97, 270, 64)] == [3, 3, 4, 4, 3, 4]
    assert {c.m for c in W.CASES} >= {47, 65, 63, 97} and {c.c for c in W.CASES} >= {16, 17, 49, 90}
    assert len(W.ALL_INSTANTIATIONS) == 46 == len(set(W.ALL_INSTANTIATIONS))


def test_every_switch_is_a_knob():
    knobs, names = W.knob_list(), W.switch_names()
    for required in ("ZSV_WINO_MIN_TILES", "ZSV_WINO_VW_MIN_WGS", "ZSV_WINOT_MIN_TILES", "ZSV_WINOT_MAX_WASTE", "ZSV_WINO_NO_F43", "ZSV_WINO_NO_X4",
                     "ZSV_WINOT_NO_F43", "ZSV_WINO_GENERIC_EPILOGUE", "ZSV_WINOT_GENERIC_EPILOGUE", "ZSV_NO_WINO"):
        assert required in names, f"the matrix no longer sets {required}"
    assert names <= knobs, f"not in ZSV_KNOB_LIST (csrc/knobs.h): {sorted(names - knobs)}"
    # the remaining switches of the issue's list are exercised on the host only (test_switches_that_leave_the_kernels)
    assert {"ZSV_WINO_NO_VW", "ZSV_WINO_NO_SPLITK", "ZSV_WINOT_NO_T32"} <= knobs


def test_the_matrix_reaches_all_46_instantiations():
    seen = {}
    for run in RUNS:
        case, direction, _, _ = run
        g = W.geometry(case, direction)
        for mode, env in W.launches(run):
            inst = W.expected_instantiation(g, direction, mode, env)
            assert inst is not None, f"{W.run_id(run)} {mode.name}: not on the Winograd kernels"
            seen.setdefault(inst[:2], []).append((W.run_id(run), mode.name, inst[2]))
    missing = [i for i in W.ALL_INSTANTIATIONS if i not in seen]
    assert not missing, f"not reached: {missing}"
    assert set(seen) == set(W.ALL_INSTANTIATIONS), f"unknown instantiations: {sorted(set(seen) - set(W.ALL_INSTANTIATIONS))}"


def test_the_edges_the_matrix_names():
    """K parts 2, 3, 4 with uneven parts; the virtual-width plans; 64 virtual-width rows; NCHUNKS = 12; two temporal segments."""
    parts = {}
    for run in RUNS:
        case, direction, vname, env = run
        g = W.geometry(case, direction)
        parts[W.run_id(run)] = W.expected_instantiation(g, direction, W.PLAIN if case.modes != "pre" else W.PRE_MODES[0], env)
    for form in ("f43", "f23"):
        for ks in (2, 3, 4):
            assert parts[f"ks_m47_c90_k3-fwd-{form}_ks{ks}"][2] == ks and parts[f"ks_m47_c90_k3-dgrad-{form}_ks{ks}"][2] == ks
    assert [(54 + ks - 1) // ks for ks in (2, 3, 4)] == [27, 18, 14] and 54 - 3 * 14 == 12           # 14/14/14/12: uneven
    assert [parts[f"ks_m97_c90_k3-fwd-f23_ks{ks}"][2] for ks in (2, 3, 4)] == [2, 3, 4]
    assert parts["vw14_m47_c16_k3-fwd-vw"][2] == 1 and parts["vw14_m47_c48_k3-fwd-vw"][2] == 2 and parts["vw7_m63_c96_k3-fwd-vw"][2] == 4
    assert parts["vw14_m64_c16_big-fwd-vw"][:2] == ("conv_wino4_kernel", (4, 0, 1, 0))
    assert parts["504_m47_c49-fwd-f43"][:2] == ("conv_wino4_kernel", (3, 12, 0, 0)) and parts["504_m47_c49-fwd-f23"][:2] == ("conv_wino_kernel", (3, 12, 1))
    widths = sorted(c.shape[3] for c in W.CASES if c.name.startswith("vw") and c.shape[:3] == (2, 2, 3) and c.kt == 1)
    assert widths == [7, 14, 15, 29, 30, 31, 61, 62, 63]
    assert [w for w in range(1, 70) if W.wino_vw_width(W.Geom((1, 16, 1, 1, w), 16, (1, 3, 3), W.ONE, (0, 1, 1)), {})] == widths
    for name, segs in (("t4_17_m47_c17", 2), ("t8_6x6_m65_c16", 2), ("t16_4x5_m63_c49", 2), ("t32_3x4_m97_c16", 2), ("t4_2x2_m63_c16", 1)):
        assert W.winot_segs(W.geometry(W.by_name(name), "fwd")) == segs


@pytest.mark.parametrize("run", RUNS, ids=[W.run_id(r) for r in RUNS])
def test_planners_agree_with_the_library(run, monkeypatch):
    lib = _lib.load()
    case, direction, _, env = run
    g = W.geometry(case, direction)
    d = _desc(g)
    for e in (env, dict(env, **W.GENERIC_ENV), dict(env, **W.OFF_ENV)):
        _setenv(monkeypatch, e)
        what = f"{W.run_id(run)} {sorted(set(e) - set(W.BASE_ENV))}"
        if "ZSV_NO_WINO" in e:
            assert not W.wino_applicable(g, direction, e)
            continue
        assert W.wino_applicable(g, direction, e), what
        if direction == "fwd":
            assert lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d)) == W.wino_workspace_bytes(g, "fwd", e), f"{what}: forward workspace"
            assert lib.zsv_conv3d_fwd_stat_tiles(ctypes.byref(d), ALIGNED_DUMMY) == W.fwd_stat_tiles_query(g, e), f"{what}: statistics tiles"
            assert lib.zsv_conv3d_fwd_add_supported(ctypes.byref(d)) == int(W.fusable(g, "fwd", e)), f"{what}: add supported"
            pre = int(lib.zsv_conv3d_pre_supported(ctypes.byref(d)))
            assert pre == int(case.modes == "pre"), f"{what}: prologue supported = {pre}"
            if pre:
                assert W.winot_geometry(g, g.cout, e), what
        else:
            assert lib.zsv_conv3d_dgrad_workspace_bytes(ctypes.byref(d)) == W.wino_workspace_bytes(g, "dgrad", e), f"{what}: input-gradient workspace"
            assert lib.zsv_conv3d_dgrad_add_supported(ctypes.byref(d)) == int(W.fusable(g, "dgrad", e)), f"{what}: add supported"


def test_switches_that_leave_the_kernels(monkeypatch):
    """ZSV_WINO_NO_VW, ZSV_WINO_NO_SPLITK and ZSV_WINOT_NO_T32 take a shape off these kernels: the restated planners say so, and the
    library's workspace answer is no longer the Winograd one."""
    lib = _lib.load()
    for name, switch in (("vw7_partial_m65_c17", "ZSV_WINO_NO_VW"), ("ks_m47_c90_k3", "ZSV_WINO_NO_SPLITK"), ("t32_3x4_m97_c16", "ZSV_WINOT_NO_T32")):
        case = W.by_name(name)
        env = dict(W.BASE_ENV, **case.variants[0][1])
        g = W.geometry(case, "fwd")
        d = _desc(g)
        _setenv(monkeypatch, env)
        on = lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d))
        assert W.wino_applicable(g, "fwd", env) and on == W.wino_workspace_bytes(g, "fwd", env)
        monkeypatch.setenv(switch, "1")
        assert not W.wino_applicable(g, "fwd", dict(env, **{switch: "1"})), f"{name}: still applicable under {switch}"
        assert lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d)) != on, f"{name}: {switch} changed nothing"
        monkeypatch.delenv(switch)


def test_a_broken_restatement_fails():
    """The workspace formula is sharp: another row-tile height, point count or part count changes the answer."""
    case = W.by_name("504_m47_c49")
    g, env = W.geometry(case, "fwd"), dict(W.BASE_ENV)
    good = W.wino_workspace_bytes(g, "fwd", env)
    assert good == W.B.align256(4 * 3 * 6 * 16 * 48 * 4)
    assert W.wino_workspace_bytes(g, "fwd", dict(env, ZSV_WINO_NO_F43="1")) == W.B.align256(4 * 3 * 4 * 16 * 48 * 4) != good
    assert W.wino_workspace_bytes(g._replace(cout=63), "fwd", env) != good
    ks = W.by_name("ks_m47_c90_k3")
    g2 = W.geometry(ks, "fwd")
    e2 = dict(W.BASE_ENV, **ks.variants[0][1])
    assert W.wino_workspace_bytes(g2, "fwd", e2) == W.wino_bytes(g2, "fwd", e2) + 2 * 3 * 47 * 2 * 7 * 12 * 4


@pytest.mark.parametrize("axis,m", [("w", 2), ("w", 4), ("t", 2), ("t", 4)])
def test_the_restated_algorithm_is_the_convolution(axis, m):
    """fp64 Winograd == fp64 convolution to rounding, forward and input gradient, and the absolute-value form dominates it; the
    input gradient's effective weights give torch's conv3d_input."""
    gen = torch.Generator().manual_seed(5)
    kernel, padding = ((3, 1, 1), (1, 0, 0)) if axis == "t" else ((3, 3, 3), (1, 1, 1))
    x = torch.randn((2, 5, 8, 3, 7), generator=gen, dtype=torch.float64)
    w = torch.randn((6, 5) + kernel, generator=gen, dtype=torch.float64)
    y = F.conv3d(x, w, None, 1, padding)
    got, got_abs = W.winograd(x, w, axis, m), W.winograd(x, w, axis, m, absolute=True)
    assert float((got - y).abs().max()) < 1e-11 and bool((got_abs >= got.abs() - 1e-11).all())
    assert bool((got_abs >= F.conv3d(x.abs(), w.abs(), None, 1, padding) * (1 - 1e-12)).all())       # the transforms amplify
    dy = torch.randn(tuple(y.shape), generator=gen, dtype=torch.float64)
    dx = torch.nn.grad.conv3d_input(x.shape, w, dy, 1, padding)
    geff = W.effective_weights(w, "dgrad")
    assert float((F.conv3d(dy, geff, None, 1, padding) - dx).abs().max()) < 1e-11
    assert float((W.winograd(dy, geff, axis, m) - dx).abs().max()) < 1e-11


@pytest.mark.parametrize("run", RUNS, ids=[W.run_id(r) for r in RUNS])
def test_preconditions(run):
    case, direction, _, env = run
    g = W.geometry(case, direction)
    form = W.form_of(g, direction, env)
    checked = 0
    for kind in W.KINDS:
        for mode in W.modes_of(case, direction):
            if kind == "normal" and mode.name in W.EXACT_ONLY:
                continue
            W.assert_preconditions(g, direction, kind, form, mode, env)
            checked += 1
    assert checked


def test_tile_sums_partition_the_tensor():
    for name in ("t4_17_m47_c17", "vw7_partial_m65_c17", "504_m47_c49"):
        case = W.by_name(name)
        g, env = W.geometry(case, "fwd"), dict(W.BASE_ENV)
        t = torch.arange(float(torch.tensor(W.out_shape(g)).prod()), dtype=torch.float64).reshape(W.out_shape(g))
        s = W.tile_sums(t, g, env)
        assert s.shape == (g.cout, W.wino_fwd_stat_tiles(g, env)) and torch.equal(s.sum(1), t.sum(dim=(0, 2, 3, 4)))
