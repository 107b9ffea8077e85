"""Host half of the tile-configuration matrix (tests/conv_config_cases.py): no GPU, needs the built library.

* the preconditions of every case, kind and configuration;
* every switch the matrix sets is a name in ZSV_KNOB_LIST (a misspelt switch would make the matrix test the default kernel);
* the tap switches take effect: under every forced (ZSV_CONV_CFG, ZSV_TAP_KS) the library's workspace and statistics-tile
  answers are the ones the restated tile table gives (the queries dereference nothing);
* the forced weight-gradient pairs are the ones the library's parsers accept, and the staged cases reach all four
  (av4, twotap) forms of every pair.
"""
import ctypes

import pytest

import conv_config_cases as C
from zeroshotvideoclassification_amd import _lib, ops

ALIGNED_DUMMY = 0x1000      # a 16-byte aligned address for the statistics-tile query, never dereferenced


def test_tables():
    assert len(C.TAP_TILES) == 6 and len(C.GENERIC_TILES) == 5 and len(C.STAGED_PAIRS) == 8 and len(C.DMA_PAIRS) == 13
    assert C.GENERIC_TILES == C.TAP_TILES[:5]
    assert sorted(C.DMA_PAIRS) == sorted([(9, 1), (9, 2), (9, 3), (8, 1), (8, 2), (8, 3), (5, 1), (5, 2), (5, 3), (4, 1), (4, 2), (4, 3), (4, 7)])
    assert not C.dma_pair_valid(9, 7) and not C.dma_pair_valid(5, 7) and not C.dma_pair_valid(7, 1) and not C.dma_pair_valid(4, 4)
    for i, bn in C.STAGED_PAIRS:
        env = C.force_env("staged", (i, bn))
        assert C.staged_pair_parsed(env["ZSV_WGRAD_CFG"], env["ZSV_WGRAD_BN"]) == (C.STAGED_ROWS[i], bn)
    assert {C.staged_pair_parsed(str(i), str(bn)) for i, bn in C.STAGED_PAIRS} == {(r, c) for r in C.STAGED_ROWS for c in C.STAGED_COLS}
    for tm, tn in C.DMA_PAIRS:
        env = C.force_env("dma", (tm, tn))
        assert C.dma_pair_valid(int(env["ZSV_WGRAD_DMA_TM"]), int(env["ZSV_WGRAD_DMA_TN"]))


def test_every_switch_is_a_knob():
    knobs = C.knob_list()
    assert len(knobs) > 40 and "ZSV_CONV_CFG" in knobs
    names = C.switch_names()
    for required in ("ZSV_CONV_CFG", "ZSV_TAP_KS", "ZSV_NO_SPLITK", "ZSV_NO_LDS_EPILOGUE", "ZSV_SPLITK_REDUCE_SCALAR", "ZSV_NO_DGRAD_S2",
                     "ZSV_WGRAD_CFG", "ZSV_WGRAD_BN", "ZSV_WGRAD_NO_TWOTAP", "ZSV_WGRAD_DMA_TM", "ZSV_WGRAD_DMA_TN", "ZSV_NO_WGRAD_WINO",
                     "ZSV_NO_WGRAD_TRING", "ZSV_WGRAD_LINEAR_WALK", "ZSV_NO_WINOT"):
        assert required in names, f"the matrix no longer sets {required}"
    assert names <= knobs, f"not in ZSV_KNOB_LIST (csrc/knobs.h): {sorted(names - knobs)}"


def test_staged_cases_reach_every_form_of_every_pair():
    for pair in C.STAGED_PAIRS:
        forms = set()
        for case, cfg, _, env in C.runs("staged"):
            if cfg != pair:
                continue
            av4, twotap = C.staged_forms(case, cfg)
            forms.add((av4, twotap and "ZSV_WGRAD_NO_TWOTAP" not in env))
        assert forms == {(a, t) for a in (False, True) for t in (False, True)}, f"pair {pair}: only {sorted(forms)}"


def test_the_dma_shapes_are_dma_shapes():
    """wgrad_dma_shape restated: stride 1, output extents = input extents, S % 16 == 0, taps * Cpad >= 256, Cin, Cout >= 16."""
    for case in C.family_cases("dma"):
        for cfg in C.configs("dma"):
            g = C.geometry(case, cfg)
            o = C.out_shape(g)
            taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
            assert g.stride == (1, 1, 1) and o[2:] == g.xs[2:] and (g.xs[2] * g.xs[3] * g.xs[4]) % 16 == 0
            assert taps <= 32 and taps * ((g.xs[1] + 15) // 16 * 16) >= 256 and g.xs[1] >= 16 and g.cout >= 16


def _modes(case):
    """(bias, relu, residual, amp, stats) of every comparison the GPU half makes on a case."""
    modes = [(case.bias, case.relu, False, 4, False)]
    if case.name == "tap_aligned":
        modes += [(True, True, False, 4, False), (True, True, True, 4, False), (False, False, False, 2, True)]
    return modes


@pytest.mark.parametrize("family", ["tap", "generic", "staged", "dma"])
def test_preconditions(family):
    seen = set()
    for case, cfg, _, _ in C.runs(family):
        g = C.geometry(case, cfg)
        for kind in C.KINDS:
            for bias, relu, residual, amp, stats in _modes(case):
                key = (g, kind, bias, relu, residual, amp)
                if key in seen:
                    continue
                seen.add(key)
                C.assert_preconditions(g, kind, bias, relu, residual, amp, stats)
    assert seen


def test_preconditions_of_the_prologue_case():
    r = C.pre_reference(C.PRE_GEOM, "exact")
    assert float(r["y_abs"].max()) < C.LIMIT and C.faces_nonzero(r["x"])
    assert (r["coef"] == r["coef"].round()).all()


# ---- the tap switches take effect -----------------------------------------------------------------------------------------
HOST_M = 130      # rows 144, 256, 160, 192, 144, 192 x columns 128, 128, 128, 128, 256, 256: pairwise different (Mp, bn)
TAP_STRIDE1 = [c for c in C.family_cases("tap") if c.stride == (1, 1, 1)]


def test_host_m_tells_the_configurations_apart():
    for m in [HOST_M] + sorted({c.xs[1] for c in TAP_STRIDE1}):
        pairs = {((m + bm - 1) // bm * bm, bn) for bm, bn in C.TAP_TILES}
        assert len(pairs) == 6, f"M = {m}: {sorted(pairs)}"


@pytest.mark.parametrize("case", TAP_STRIDE1, ids=[c.name for c in TAP_STRIDE1])
def test_tap_switches_take_effect(case, monkeypatch):
    lib = _lib.load()
    n, cin, t, h, w = case.xs
    taps = case.kernel[0] * case.kernel[1] * case.kernel[2]
    d = ops.conv_desc(case.xs, (HOST_M, cin) + case.kernel, case.stride, case.padding)
    out_elems = n * HOST_M * d.To * d.Ho * d.Wo
    in_elems = n * cin * t * h * w
    p = n * d.To * d.Ho * d.Wo
    stats_possible = (d.To * d.Ho * d.Wo) % 4 == 0
    answers = set()
    for cfg in range(6):
        for ks in (None, 1, 2, 4, 27, 99):
            monkeypatch.setenv("ZSV_CONV_CFG", str(cfg))
            if ks is None:
                monkeypatch.setenv("ZSV_NO_SPLITK", "1")
                monkeypatch.delenv("ZSV_TAP_KS", raising=False)
            else:
                monkeypatch.delenv("ZSV_NO_SPLITK", raising=False)
                monkeypatch.setenv("ZSV_TAP_KS", str(ks))
            what = f"{case.name} cfg {cfg} ks {ks}"
            fwd = lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d))
            assert fwd == C.tap_workspace_bytes(HOST_M, cin, taps, out_elems, cfg, ks or 1), f"{what}: forward workspace {fwd}"
            dg = lib.zsv_conv3d_dgrad_workspace_bytes(ctypes.byref(d))
            assert dg == C.tap_workspace_bytes(cin, HOST_M, taps, in_elems, cfg, ks or 1), f"{what}: input-gradient workspace {dg}"
            tiles = lib.zsv_conv3d_fwd_stat_tiles(ctypes.byref(d), ALIGNED_DUMMY)
            bn = C.TAP_TILES[cfg][1]
            split = max(1, min(ks or 1, taps * ((cin + 15) // 16))) > 1
            assert tiles == ((p + bn - 1) // bn if stats_possible and not split else 0), f"{what}: {tiles} statistics tiles"
            if ks is None:
                answers.add((fwd, dg, tiles))
    # 64x128 and 64x256 pad the rows alike: only the statistics tiles tell them apart, where the shape has them and P > 128
    told_apart = 6 if stats_possible and (p + 127) // 128 != (p + 255) // 256 else 5
    assert len(answers) == told_apart, f"{case.name}: the six configurations give only {len(answers)} different answers"


def test_a_broken_restatement_fails():
    """The formula is sharp: one row more or less in the restated table changes the answer."""
    good = C.tap_workspace_bytes(130, 32, 3, 1000, 0, 1)
    assert good == C.align256((3 * 32 + 16) * 144 * 4)
    assert C.tap_workspace_bytes(145, 32, 3, 1000, 0, 1) != good and C.tap_workspace_bytes(130, 32, 3, 1000, 1, 1) != good
    assert C.tap_workspace_bytes(130, 32, 3, 1000, 0, 2) == good + 2 * 1000 * 4
