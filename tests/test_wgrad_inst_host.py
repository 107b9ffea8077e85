"""Host half of the weight-gradient instantiation matrix (tests/wgrad_inst_cases.py): no GPU, needs the built library.

* under every (row, switches), forced slice counts included, the restated planners give the library's own answers: the workspace
  bytes (which pin the slice count and the tile choice), the mask bytes and ``zsv_conv3d_pre_supported`` (the queries dereference
  nothing);
* the expected instantiations over the whole matrix are all 21, so a retune that moves a row off its kernel fails here;
* every switch the matrix sets is a name in ZSV_KNOB_LIST;
* the preconditions of every launch, in both operand kinds;
* the fp64 restatement of the Winograd forms is the weight gradient, and its absolute-value form dominates it;
* the checker rejects planted errors: a border voxel dropped, a chunk counted twice, an F(4,3) result moved by two bounds.
"""
import ctypes

import pytest
import torch
from torch.nn.grad import conv3d_weight

import wgrad_inst_cases as G
from zeroshotvideoclassification_amd import _lib, ops

RUNS = G.runs()


def _desc(g):
    return ops.conv_desc(g.xs, (g.cout, g.xs[1]) + g.kernel, g.stride, g.padding)


def _setenv(monkeypatch, env):
    for name in G.switch_names() - set(env):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _envs(run):
    """The switch sets a run launches under: its own and, on the Winograd / ring rows, the forced slice counts."""
    return [run.env] + ([dict(run.env, **{run.row.slices: str(s)}) for s in G.FORCED_SLICES] if run.row.slices else [])


def test_the_table_of_instantiations():
    assert len(G.ALL_INSTANTIATIONS) == 21 == len(set(G.ALL_INSTANTIATIONS))
    assert [G.rows_144_or_128(n) for n in (100, 130, 197, 257, 144, 129)] == [128, 144, 128, 144, 144, 144]
    assert [G.pad_144_or_128(n) for n in (100, 130, 197, 257)] == [128, 144, 256, 288]
    # "tile + 1 row" is refused: 145 rows pad to 256 / 288, far above 30 %
    g = G.by_name("s32_m130").geom
    assert G.wgrad_wino_shape(g, {}) and not G.wgrad_wino_shape(g._replace(cout=145), {})


def test_every_switch_is_a_knob():
    knobs, names = G.knob_list(), G.switch_names()
    for required in ("ZSV_NO_WGRAD_WINO4", "ZSV_NO_WGRAD_TWINO", "ZSV_WGRAD_WINO_SLICES", "ZSV_WGRAD_TRING_SLICES", "ZSV_STEM_WGRAD_WGS",
                     "ZSV_WGRAD_WGS", "ZSV_WGRAD_DMA_SLICES"):
        assert required in names, f"the matrix no longer sets {required}"
    assert names <= knobs, f"not in ZSV_KNOB_LIST (csrc/knobs.h): {sorted(names - knobs)}"
    # the switches the restated planners read without the matrix setting them
    assert {"ZSV_NO_WINO", "ZSV_NO_WGRAD_WINO", "ZSV_NO_WGRAD_TRING", "ZSV_NO_WGRAD_DMA", "ZSV_NO_STEM_WGRAD", "ZSV_NO_T2_DENSE",
            "ZSV_NO_BN_FUSION"} <= knobs


def test_the_matrix_reaches_all_21_instantiations():
    seen = {}
    for run in RUNS:
        inst = G.expected_instantiation(run.row.geom, run.env, run.pre)
        assert inst is not None, f"{G.run_id(run)}: not on a kernel of the matrix"
        seen.setdefault(inst, []).append(G.run_id(run))
    missing = [i for i in G.ALL_INSTANTIATIONS if i not in seen]
    assert not missing, f"not reached: {missing}"
    assert set(seen) == set(G.ALL_INSTANTIATIONS), f"unknown instantiations: {sorted(set(seen) - set(G.ALL_INSTANTIATIONS))}"
    print(f"{len(seen)} instantiations reached by {len(RUNS)} runs")
    for inst in G.ALL_INSTANTIATIONS:
        print(f"  {inst[0]}<{','.join(str(v) for v in inst[1])}>: {' '.join(seen[inst])}")


def test_the_rows_reach_what_they_name():
    inst = {G.run_id(r): G.expected_instantiation(r.row.geom, r.env, r.pre) for r in RUNS}
    w, w4 = "conv_wgrad_wino_kernel", "conv_wgrad_wino4_kernel"
    for rid, want in (("s32_m50-default-plain", (w, (4, 2, 0))), ("s32_m100-default-plain", (w4, (4, 4))), ("s32_m100-f23-plain", (w, (8, 1, 0))),
                      ("s32_m130-default-plain", (w4, (5, 4))), ("s32_m130-f23-plain", (w, (9, 1, 0))), ("s32_m197-default-plain", (w4, (4, 4))),
                      ("s32_m257-f23-plain", (w, (9, 1, 0))), ("e14_m130-default-plain", (w, (9, 1, 1))), ("e14_m50-default-plain", (w, (4, 2, 1))),
                      ("e20x12_m100-default-plain", (w, (8, 1, 1))), ("s32_k3_m130-default-plain", (w4, (5, 4))),
                      ("t2_k3_m100-f23-plain", (w, (8, 1, 0))),
                      ("t4_c100-default-pre", ("conv_wgrad_tring_kernel", (8, 1))), ("t4_c130-default-pre", ("conv_wgrad_tring_kernel", (9, 1))),
                      ("t8_c100-wino-pre", ("conv_wgrad_twino_kernel", (8, 1))), ("t8_c130-wino-pre", ("conv_wgrad_twino_kernel", (9, 1))),
                      ("t8_c130-ring-plain", ("conv_wgrad_tring_kernel", (9, 0))), ("t4_c197_m50-default-plain", ("conv_wgrad_tring_kernel", (8, 0))),
                      ("t4_c257_m50-default-pre", ("conv_wgrad_tring_kernel", (9, 1))),
                      ("gen_small_m45-default-plain", ("conv_wgrad_generic_kernel", (4, 2, 1, 4))),
                      ("gen_small_m80-default-plain", ("conv_wgrad_generic_kernel", (4, 4, 2, 2))),
                      ("gen_sliced_m144-default-plain", ("conv_wgrad_generic_kernel", (9, 1, 1, 4))),
                      ("stem_m20-parts1-plain", ("stem_wgrad_kernel", ())), ("t2_ragged-default-plain", ("t2_fold_kernel", ()))):
        assert inst[rid] == want, f"{rid}: {inst[rid]}"
    # two row tiles, the second ragged; one slice without a workspace and several; the stem's parts
    assert G.wgrad_wino_plan(G.by_name("s32_m197").geom, G.BASE_ENV)[2] == 2 and G.wgrad_wino4_plan(G.by_name("s32_m257").geom, G.BASE_ENV)[2] == 2
    assert G.wgrad_tring_tiles(G.by_name("t4_c197_m50").geom) == (8, 2, 1) and G.wgrad_tring_tiles(G.by_name("t4_c257_m50").geom) == (9, 2, 1)
    assert [G.wgrad_gen_plan(G.by_name(f"gen_small_m{m}").geom)[1].slices for m in (45, 80, 144)] == [1, 1, 1]
    assert all(G.wgrad_gen_plan(G.by_name(f"gen_sliced_m{m}").geom)[1].slices > 1 for m in (45, 80, 144))
    stem = G.by_name("stem_m20")
    assert [G.stem_wgrad_parts(stem.geom, dict(venv)) for _, venv in stem.variants] == [2, 1]
    assert G.stem_wgrad_parts(G.by_name("stem_tiny").geom, {}) == 1


@pytest.mark.parametrize("run", RUNS, ids=[G.run_id(r) for r in RUNS])
def test_planners_agree_with_the_library(run, monkeypatch):
    lib = _lib.load()
    g = run.row.geom
    d = _desc(g)
    counts = []
    for env in _envs(run):
        _setenv(monkeypatch, env)
        what = f"{G.run_id(run)} {sorted(set(env) - set(G.BASE_ENV))}"
        assert int(lib.zsv_conv3d_wgrad_workspace_bytes(ctypes.byref(d))) == G.workspace_bytes(g, env), f"{what}: workspace bytes"
        assert int(lib.zsv_conv3d_wgrad_mask_bytes(ctypes.byref(d))) == G.mask_bytes(g, env), f"{what}: mask bytes"
        assert int(lib.zsv_conv3d_pre_supported(ctypes.byref(d))) == int(G.pre_supported(g, env)), f"{what}: prologue supported"
        if run.row.slices:
            counts.append(G.planned_slices(g, env))
    if run.row.slices:
        assert G.mask_bytes(g, run.env) != 0 if G.route(g, run.env) == "wino" else G.pre_supported(g, run.env), G.run_id(run)
        assert counts[1] == 1 and counts[2] == 7, f"{G.run_id(run)}: forced slice counts {counts[1:]}"
    if run.pre:
        assert G.pre_supported(g, run.env)


def test_a_broken_restatement_fails():
    """The workspace formula is sharp: another slice count, point count or row tile changes the answer."""
    g, env = G.by_name("s32_m130").geom, dict(G.BASE_ENV)
    kp = 3 * 32
    p2, p4 = G.wgrad_wino_plan(g, env), G.wgrad_wino4_plan(g, env)
    assert G.wgrad_wino_workspace_bytes(g, env) == max(G.align256(p2.slices * 4 * 130 * kp * 4), G.align256(p4.slices * 6 * 130 * kp * 4)) + 4096 * 4
    one = dict(env, ZSV_WGRAD_WINO_SLICES="1")
    assert G.wgrad_wino_workspace_bytes(g, one) == G.align256(6 * 130 * kp * 4) + 4096 * 4 != G.wgrad_wino_workspace_bytes(g, env)
    t = G.by_name("t8_c130").geom
    seven = dict(env, ZSV_WGRAD_TRING_SLICES="7")
    assert G.wgrad_tring_workspace_bytes(t, seven) == 7 * 130 * 4 * 100 * 4          # the Winograd form's four points are the larger
    assert G.wgrad_tring_workspace_bytes(G.by_name("t4_c130").geom, seven) == 7 * 130 * 3 * 100 * 4


@pytest.mark.parametrize("axis,m", [("w", 2), ("w", 4), ("t", 2)])
def test_the_restated_forms_are_the_weight_gradient(axis, m):
    gen = torch.Generator().manual_seed(11)
    g = G.Geom((2, 5, 4, 3, 8), 6, (3, 3, 3), G.ONE, (1, 1, 1)) if axis == "w" else G.Geom((2, 5, 4, 3, 8), 6, (3, 1, 1), G.ONE, (1, 0, 0))
    x = torch.randn(g.xs, generator=gen, dtype=torch.float64)
    dy = torch.randn(G.out_shape(g), generator=gen, dtype=torch.float64)
    dw = conv3d_weight(x, (6, 5) + g.kernel, dy, 1, g.padding)
    got, _ = G.winograd_wgrad(x, dy, g, axis, m)
    got_abs, peak = G.winograd_wgrad(x, dy, g, axis, m, absolute=True)
    assert got.shape == dw.shape and float((got - dw).abs().max()) < 1e-11
    assert bool((got_abs >= got.abs() - 1e-11).all()) and peak > 0
    assert bool((got_abs >= conv3d_weight(x.abs(), (6, 5) + g.kernel, dy.abs(), 1, g.padding) * (1 - 1e-12)).all())       # the transforms amplify


@pytest.mark.parametrize("run", RUNS, ids=[G.run_id(r) for r in RUNS])
def test_preconditions(run):
    g = run.row.geom
    form = G.form_of(g, run.env, run.pre)
    for kind in G.KINDS:
        G.assert_preconditions(g, kind, form, run.pre)
        r = G.reference(g, kind, form, run.pre)
        assert bool((r["abs"] >= r["dw"].abs() * (1 - 1e-12)).all())
        if kind == "normal":
            assert G.c_round(g, form, run.pre) >= G.C_FIRST[form] + 1 and bool((r["bound"] >= 0).all())


def test_the_checker_rejects_planted_errors():
    g = G.by_name("s32_m130").geom
    x, _, _, _, dy = G.operands(g, "exact", amp=G.AMP)
    wshape = (g.cout, g.xs[1]) + g.kernel
    ref = G.reference(g, "exact", "f23w")
    assert G.compare("the reference itself", ref["dw"].float(), ref, "exact") == 0.0
    # one border voxel dropped
    x2 = x.clone()
    assert float(x2[1, 3, 0, 0, 31]) != 0
    x2[1, 3, 0, 0, 31] = 0
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.compare("dropped voxel", conv3d_weight(x2, wshape, dy, 1, g.padding).float(), ref, "exact")
    # one 32-voxel chunk (a row of clip 2) counted twice
    dy2 = dy.clone()
    dy2[2, :, 1, 5, :] *= 2
    with pytest.raises(AssertionError, match="differ from the exact result"):
        G.compare("doubled chunk", conv3d_weight(x, wshape, dy2, 1, g.padding).float(), ref, "exact")
    # F(4,3) in the exact kind: within the emit bound, not bit for bit; two bounds off is rejected
    ref4 = G.reference(g, "exact", "f43w")
    assert ref4["bound"] is not None and float(ref4["bound"].max()) < 0.5
    inside = (ref4["dw"] + 0.9 * ref4["bound"]).float()
    assert G.compare("inside", inside, ref4, "exact") <= 1.0
    moved = ref4["dw"].clone()
    moved[7, 3, 0, 1, 2] += 2 * ref4["bound"][7, 3, 0, 1, 2]
    with pytest.raises(AssertionError, match="beyond the bound"):
        G.compare("moved by two bounds", moved.float(), ref4, "exact")
    # the normal kind's bound is per element: an element of a small-magnitude row moved by two of ITS bounds fails
    refn = G.reference(g, "normal", "f23w")
    moved = refn["dw"].clone()
    i = int(refn["bound"].flatten().argmin())
    moved.view(-1)[i] += 2 * refn["bound"].view(-1)[i]
    with pytest.raises(AssertionError, match="beyond the bound"):
        G.compare("moved by two bounds", moved.float(), refn, "normal")
