"""Every tile configuration of the fp32 convolution kernels, forced on the smallest shapes that cross its tile edges, against an
fp64 reference with a derived per-element bound (tests/conv_config_cases.py: cases, operands, references, bounds).

Each case runs forward, input gradient and weight gradient through ``ops.conv3d`` autograd under the forcing switches, in both
operand kinds; the epilogue modes of the tap kernel and the guard-band runs go through the C ABI.  Every test prints its worst
error / bound ratio (0 in the ``exact`` kind, where the comparison is ``torch.equal``).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_config_cases as C  # noqa: E402
from guarded import guarded, guarded_like  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _setenv(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _dev(t):
    return None if t is None else t.float().to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _desc(g):
    return ops.conv_desc(g.xs, (g.cout, g.xs[1]) + g.kernel, g.stride, g.padding)


def _autograd(g, kind, bias, relu, what):
    """Forward, input gradient and weight gradient of ``g`` through ops.conv3d; returns the worst ratios and the three results."""
    r = C.reference(g, kind, bias, relu)
    x, w, b = _dev(r["x"]).requires_grad_(), _dev(r["w"]).requires_grad_(), _dev(r["b"])
    y = ops.conv3d(x, w, b, g.stride, g.padding, relu=relu)
    y.backward(_dev(r["dy"]))
    torch.cuda.synchronize()
    ratios = {"y": C.check(f"{what}: forward", y, r["y"], r["y_bound"], kind),
              "dx": C.check(f"{what}: input gradient", x.grad, r["dx"], r["dx_bound"], kind),
              "dw": C.check(f"{what}: weight gradient", w.grad, r["dw"], r["dw_bound"], kind)}
    print(f"{what}: worst error / bound  y {ratios['y']:.3f}  dx {ratios['dx']:.3f}  dw {ratios['dw']:.3f}")
    return ratios, (y.detach(), x.grad, w.grad)


def _out(shape, guard):
    """An output of exactly ``shape``: NaN-filled, between guard bands when ``guard``."""
    if guard:
        buf = guarded_like(torch.float32, shape, DEV, 0xFF)
        return buf.view(torch.float32, tuple(shape)), buf
    return torch.full(tuple(shape), NAN, device=DEV), None


def _work(nbytes, guard):
    """A workspace of exactly the queried size (between guard bands when ``guard``): (address, keep-alive)."""
    if guard:
        buf = guarded(nbytes, DEV, 0xFF)
        return buf.ptr, buf
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)
    return ws.data_ptr(), ws


def _fwd_abi(g, x, w, b=None, res=None, relu=False, stats=False, guard=False, what="forward"):
    lib = _lib.load()
    d = _desc(g)
    y, ybuf = _out(C.out_shape(g), guard)
    nbytes = int(lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d)))
    ws, wbuf = _work(nbytes, guard)
    tiles, st = 0, None
    if stats:
        tiles = int(lib.zsv_conv3d_fwd_stat_tiles(ctypes.byref(d), y.data_ptr()))
        if tiles == 0:
            return None, None
        st = torch.full((2, g.cout, tiles), NAN, device=DEV)
    _lib.check(lib.zsv_conv3d_fwd_full(ctypes.byref(d), x.data_ptr(), w.data_ptr(), _ptr(b), _ptr(res), y.data_ptr(), 1 if relu else 0,
                                       _ptr(st), tiles, ws, nbytes, None), what)
    torch.cuda.synchronize()
    if guard:
        ybuf.check(f"{what}: y")
        wbuf.check(f"{what}: workspace")
    return y, st


def _dgrad_abi(g, dy, w, guard=False, what="input gradient"):
    lib = _lib.load()
    d = _desc(g)
    dx, xbuf = _out(g.xs, guard)
    nbytes = int(lib.zsv_conv3d_dgrad_workspace_bytes(ctypes.byref(d)))
    ws, wbuf = _work(nbytes, guard)
    _lib.check(lib.zsv_conv3d_dgrad(ctypes.byref(d), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), ws, nbytes, None), what)
    torch.cuda.synchronize()
    if guard:
        xbuf.check(f"{what}: dx")
        wbuf.check(f"{what}: workspace")
    return dx


def _wgrad_abi(g, x, dy, guard=False, what="weight gradient"):
    lib = _lib.load()
    d = _desc(g)
    dw, dbuf = _out((g.cout, g.xs[1]) + g.kernel, guard)
    nbytes = int(lib.zsv_conv3d_wgrad_workspace_bytes(ctypes.byref(d)))
    ws, wbuf = _work(nbytes, guard)
    _lib.check(lib.zsv_conv3d_wgrad(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws, nbytes, None), what)
    torch.cuda.synchronize()
    if guard:
        dbuf.check(f"{what}: dw")
        wbuf.check(f"{what}: workspace")
    return dw


# ---- the matrix: every case x configuration x variant x kind through autograd ------------------------------------------------
ROWS = [(case, cfg, vname, env, kind) for case, cfg, vname, env in C.all_runs() for kind in C.KINDS]


def _row_id(row):
    case, cfg, vname, _, kind = row
    return f"{case.name}-{C.config_id(cfg)}-{vname}-{kind}"


@pytest.mark.parametrize("row", ROWS, ids=[_row_id(r) for r in ROWS])
def test_forced_configuration(row, monkeypatch):
    case, cfg, _, env, kind = row
    _setenv(monkeypatch, env)
    _autograd(C.geometry(case, cfg), kind, case.bias, case.relu, _row_id(row))


# ---- the tap kernel's epilogue modes on the aligned shape ------------------------------------------------------------------
ALIGNED = C.by_name("tap_aligned")
MODE_ROWS = [(cfg, vname, venv, kind) for cfg in C.configs("tap") for vname, venv in ALIGNED.variants for kind in C.KINDS]


@pytest.mark.parametrize("cfg,vname,venv,kind", MODE_ROWS, ids=[f"{C.config_id(c)}-{v}-{k}" for c, v, _, k in MODE_ROWS])
def test_tap_epilogue_modes(cfg, vname, venv, kind, monkeypatch):
    """bias + ReLU, bias + residual + ReLU, the statistics epilogue and the BatchNorm + ReLU prologue, with the LDS-transposed
    epilogue and with the plain one (which has no statistics: the query must then say 0 tiles)."""
    lib = _lib.load()
    _setenv(monkeypatch, dict(C.force_env("tap", cfg), **ALIGNED.env, **venv))
    g = C.geometry(ALIGNED, cfg)
    what = f"tap_aligned-{C.config_id(cfg)}-{vname}-{kind}"
    ratios = {}
    for mode, residual in (("bias_relu", False), ("bias_residual_relu", True)):
        r = C.reference(g, kind, True, True, residual)
        y, _ = _fwd_abi(g, _dev(r["x"]), _dev(r["w"]), _dev(r["b"]), _dev(r["res"]), relu=True, what=f"{what}: {mode}")
        ratios[mode] = C.check(f"{what}: {mode}", y, r["y"], r["y_bound"], kind)

    # statistics: per channel and column tile the sum of y and of y^2 of the raw convolution; summed over the tiles in fp64
    r = C.reference(g, kind, amp=2)
    if kind == "exact":
        C.assert_preconditions(g, kind, amp=2, stats=True)
    y, st = _fwd_abi(g, _dev(r["x"]), _dev(r["w"]), stats=True, what=f"{what}: statistics")
    o = C.out_shape(g)
    p = o[0] * o[2] * o[3] * o[4]
    if vname == "plain":
        assert st is None, "the plain epilogue has no statistics"
    else:
        assert st is not None and st.shape[2] == (p + C.TAP_TILES[cfg][1] - 1) // C.TAP_TILES[cfg][1]
        ratios["stats_y"] = C.check(f"{what}: statistics, y", y, r["y"], r["y_bound"], kind)
        assert not bool(torch.isnan(st).any()), f"{what}: a statistics entry was not written"
        s1, s2 = st[0].double().sum(1).cpu(), st[1].double().sum(1).cpu()
        ref1, ref2 = r["y"].sum(dim=(0, 2, 3, 4)), (r["y"] * r["y"]).sum(dim=(0, 2, 3, 4))
        if kind == "exact":
            assert torch.equal(s1, ref1) and torch.equal(s2, ref2), f"{what}: the statistics are not the exact sums"
        else:
            b1, b2 = (p + 2) * C.U * r["y_abs"].sum(dim=(0, 2, 3, 4)), (p + 2) * C.U * (r["y_abs"] * r["y_abs"]).sum(dim=(0, 2, 3, 4))
            ratios["sum_y"], ratios["sum_y2"] = float(((s1 - ref1).abs() / b1).max()), float(((s2 - ref2).abs() / b2).max())
            assert ratios["sum_y"] <= 1 and ratios["sum_y2"] <= 1, f"{what}: statistics beyond the bound: {ratios}"

    # the prologue: on this shape if the library supports it there, else on the smallest temporal shape it supports
    _setenv(monkeypatch, C.PRE_ENV)
    gp = g if lib.zsv_conv3d_pre_supported(ctypes.byref(_desc(g))) else C.PRE_GEOM
    d = _desc(gp)
    assert lib.zsv_conv3d_pre_supported(ctypes.byref(d)), "the prologue shape is not supported"
    r = C.pre_reference(gp, kind)
    assert kind != "exact" or float(r["y_abs"].max()) < C.LIMIT
    x, w, coef = _dev(r["x"]), _dev(r["w"]), _dev(r["coef"])
    y = torch.full(C.out_shape(gp), NAN, device=DEV)
    nbytes = int(lib.zsv_conv3d_fwd_workspace_bytes(ctypes.byref(d)))
    taps = gp.kernel[0] * gp.kernel[1] * gp.kernel[2]
    assert nbytes == C.tap_workspace_bytes(gp.cout, gp.xs[1], taps, y.numel(), cfg, 1), "the prologue case is not on the forced tap tile"
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.zsv_conv3d_fwd_pre(ctypes.byref(d), x.data_ptr(), coef.data_ptr(), coef.shape[1], w.data_ptr(), y.data_ptr(), None, 0,
                                      ws.data_ptr(), nbytes, None), "zsv_conv3d_fwd_pre")
    torch.cuda.synchronize()
    ratios["prologue"] = C.check(f"{what}: prologue", y, r["y"], r["y_bound"], kind)
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ---- guard bands: one run per configuration on the first ragged case of each family ---------------------------------------------
GUARD_ROWS = [(family, cfg) for family in ("tap", "generic", "staged", "dma") for cfg in C.configs(family)]


@pytest.mark.parametrize("family,cfg", GUARD_ROWS, ids=[f"{f}-{C.config_id(c)}" for f, c in GUARD_ROWS])
def test_forced_configuration_stays_inside_its_buffers(family, cfg, monkeypatch):
    """The output in a buffer of exactly its size, the workspace of exactly the size queried under the forced switches, both
    between guard bands: a ragged tile that writes past its rows or columns is an assertion inside the test's own allocation."""
    case = C.family_cases(family)[0]
    _setenv(monkeypatch, dict(C.force_env(family, cfg), **case.env))
    g = C.geometry(case, cfg)
    what = f"{case.name}-{C.config_id(cfg)}"
    r = C.reference(g, "exact", case.bias, case.relu)
    x, w, dy = _dev(r["x"]), _dev(r["w"]), _dev(r["dy"])
    if family in ("tap", "generic"):
        y, _ = _fwd_abi(g, x, w, guard=True, what=f"{what}: forward")
        C.check(f"{what}: forward", y, r["y"], r["y_bound"], "exact")
        dx = _dgrad_abi(g, dy, w, guard=True, what=f"{what}: input gradient")
        C.check(f"{what}: input gradient", dx, r["dx"], r["dx_bound"], "exact")
    else:
        dw = _wgrad_abi(g, x, dy, guard=True, what=f"{what}: weight gradient")
        C.check(f"{what}: weight gradient", dw, r["dw"], r["dw_bound"], "exact")


# ---- reproducibility: once per family -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["tap", "generic", "staged", "dma"])
def test_forced_configuration_is_reproducible(family, monkeypatch):
    case, cfg, vname, env = C.runs(family)[0]
    _setenv(monkeypatch, env)
    g = C.geometry(case, cfg)
    _, first = _autograd(g, "normal", case.bias, case.relu, f"{case.name}-{C.config_id(cfg)} (first run)")
    _, second = _autograd(g, "normal", case.bias, case.relu, f"{case.name}-{C.config_id(cfg)} (second run)")
    for name, a, b in zip(("forward", "input gradient", "weight gradient"), first, second):
        assert torch.equal(a, b), f"{case.name}: the {name} is not bitwise reproducible"
