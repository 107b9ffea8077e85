"""Every instantiation of the Winograd-form forward / input-gradient kernels (csrc/conv_wino.hip), forced on the smallest shapes that
cross its edges, against an fp64 reference: bit for bit on exactly representable operands, within a derived per-element bound on
standard-normal ones (tests/wino_cases.py: cases, restated planners, operands, references, bounds).

Every launch goes through the C ABI (zsv_conv3d_fwd_full, zsv_conv3d_fwd_pre, zsv_conv3d_dgrad_add) under the forcing switches,
with the output, the workspace of exactly the queried size and the statistics between guard bands, NaN-filled.  Each mode runs with
the compiled-in epilogue and again under the generic-epilogue switches: both do the same arithmetic on y (conv_wino4_kernel: one
output transform, then + add, + bias, max(., 0) in that order in either form), so y must agree bit for bit; the statistics may
differ in the order of their sums and are each compared with the reference.  Every test prints the kernel it expects and its worst
error / bound ratio (0 in the ``exact`` kind, where the comparison is ``torch.equal``).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import wino_cases as W  # noqa: E402
from guarded import guarded, guarded_like  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ops  # noqa: E402

DEV = "cuda"
ZSV_E_UNSUPPORTED = 6                 # include/zsv_hip.h


def _setenv(monkeypatch, env):
    """Exactly ``env`` of the matrix's switches: the others are unset (a generic-epilogue switch left over from the launch before
    would turn every later launch into the generic form)."""
    for name in W.switch_names() - set(env):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _dev(t):
    return None if t is None else t.float().to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _desc(g):
    return ops.conv_desc(g.xs, (g.cout, g.xs[1]) + g.kernel, g.stride, g.padding)


def _out(shape):
    buf = guarded_like(torch.float32, shape, DEV, 0xFF)          # 0xFF bytes: NaN
    return buf.view(torch.float32, tuple(shape)), buf


class Launcher:
    """The device operands of one (geometry, direction, kind) and the three entry points on them."""

    def __init__(self, g, direction, kind):
        self.g, self.direction, self.d, self.lib = g, direction, _desc(g), _lib.load()
        o = W.operands(g, direction, kind)
        self.inp, self.w, self.add, self.coef = _dev(o["inp"]), _dev(o["w"]), _dev(o["add"]), _dev(o["coef"])
        m = W.rows_and_channels(g, direction)[0]
        self.out_shape = (g.xs[0], m) + tuple(g.xs[2:])

    def launch(self, mode, bias, what, stat_tiles=None):
        """(status, y, statistics [2][M][tiles] or None); the guard bands are checked when the call succeeded."""
        lib, d = self.lib, ctypes.byref(self.d)
        y, ybuf = _out(self.out_shape)
        bufs = [(ybuf, "output")]
        if self.direction == "dgrad":
            nbytes = int(lib.zsv_conv3d_dgrad_workspace_bytes(d))
            ws = guarded(nbytes, DEV, 0xFF)
            status = lib.zsv_conv3d_dgrad_add(d, self.inp.data_ptr(), self.w.data_ptr(), _ptr(self.add if mode.add else None), y.data_ptr(),
                                              ws.ptr, nbytes, None)
            st = None
        else:
            nbytes = int(lib.zsv_conv3d_fwd_workspace_bytes(d))
            ws = guarded(nbytes, DEV, 0xFF)
            tiles, st = 0, None
            if mode.stats:
                tiles = int(lib.zsv_conv3d_fwd_stat_tiles(d, y.data_ptr())) if stat_tiles is None else stat_tiles
                st, sbuf = _out((2, self.g.cout, max(tiles, 1)))
                bufs.append((sbuf, "statistics"))
            if mode.pre:
                status = lib.zsv_conv3d_fwd_pre(d, self.inp.data_ptr(), self.coef.data_ptr(), self.coef.shape[1], self.w.data_ptr(), y.data_ptr(),
                                                _ptr(st), tiles, ws.ptr, nbytes, None)
            else:
                status = lib.zsv_conv3d_fwd_full(d, self.inp.data_ptr(), self.w.data_ptr(), _ptr(_dev(bias)), _ptr(self.add if mode.add else None),
                                                 y.data_ptr(), 1 if mode.relu else 0, _ptr(st), tiles, ws.ptr, nbytes, None)
        torch.cuda.synchronize()
        if status == 0:
            for buf, name in bufs + [(ws, "workspace")]:
                buf.check(f"{what}: {name}")
        return status, y, st


def _compare(what, kind, g, form, env, mode, r, y, st, ratios):
    ratios["y"] = max(ratios.get("y", 0.0), W.check(f"{what}: y", y, r["y"], r["bound"], kind))
    if mode.stats:
        s = W.stat_reference(g, kind, form, env, mode.pre)
        assert st.shape[2] == s["sum"].shape[1], f"{what}: {st.shape[2]} statistics tiles, {s['sum'].shape[1]} expected"
        ratios["sum_y"] = max(ratios.get("sum_y", 0.0), W.check(f"{what}: sum y", st[0], s["sum"], s["sum_bound"], kind))
        ratios["sum_y2"] = max(ratios.get("sum_y2", 0.0), W.check(f"{what}: sum y^2", st[1], s["sq"], s["sq_bound"], kind))


# ---- the matrix -------------------------------------------------------------------------------------------------------------
ROWS = [(run, kind) for run in W.runs() for kind in W.KINDS]


def _row_id(row):
    return f"{W.run_id(row[0])}-{row[1]}"


@pytest.mark.parametrize("row", ROWS, ids=[_row_id(r) for r in ROWS])
def test_forced_instantiation(row, monkeypatch):
    run, kind = row
    case, direction, _, env = run
    g = W.geometry(case, direction)
    form = W.form_of(g, direction, env)
    L = Launcher(g, direction, kind)
    ratios, kernels, first = {}, set(), None
    for mode in W.modes_of(case, direction):
        if kind == "normal" and mode.name in W.EXACT_ONLY:
            continue
        r = W.reference(g, direction, kind, form, mode)
        got = []
        for label, e in (("compiled-in epilogue", env), ("generic epilogue", dict(env, **W.GENERIC_ENV))):
            _setenv(monkeypatch, e)
            what = f"{_row_id(row)}: {mode.name}, {label}"
            inst = W.expected_instantiation(g, direction, mode, e)
            kernels.add(f"{inst[0]}<{','.join(str(v) for v in inst[1])}>x{inst[2]}")
            status, y, st = L.launch(mode, r["bias"], what)
            _lib.check(status, what)
            _compare(what, kind, g, form, e, mode, r, y, st, ratios)
            got.append(y)
            if first is None:
                first = (mode, r["bias"], y)
        assert torch.equal(got[0], got[1]), f"{_row_id(row)}: {mode.name}: the compiled-in and the generic epilogue differ"
    _setenv(monkeypatch, env)

    # one repeat: bitwise reproducible
    mode, bias, y0 = first
    status, y1, _ = L.launch(mode, bias, f"{_row_id(row)}: repeat")
    _lib.check(status, "repeat")
    assert torch.equal(y0, y1), f"{_row_id(row)}: {mode.name} is not bitwise reproducible"

    # what the queries call unsupported is refused: the epilogue extras with K parts; residual + statistics always
    if kind == "exact":
        fusable = W.fusable(g, direction, env)
        if direction == "dgrad":
            assert int(L.lib.zsv_conv3d_dgrad_add_supported(ctypes.byref(L.d))) == int(fusable)
            refused = [] if fusable else [W.DGRAD_MODES[1]]
        else:
            assert int(L.lib.zsv_conv3d_fwd_add_supported(ctypes.byref(L.d))) == int(fusable)
            assert int(L.lib.zsv_conv3d_fwd_stat_tiles(ctypes.byref(L.d), None)) == W.fwd_stat_tiles_query(g, env)
            refused = [W.REFUSED] if case.modes != "pre" else []
            if not fusable:
                refused += [W.FWD_MODES[4], W.FWD_MODES[1]]
        for mode in refused:
            status, _, _ = L.launch(mode, None, "refused", stat_tiles=W.wino_fwd_stat_tiles(g, env) if direction == "fwd" else None)
            assert status == ZSV_E_UNSUPPORTED, f"{_row_id(row)}: {mode.name} returned {status}, not ZSV_E_UNSUPPORTED"

        # the Winograd-off result (the direct kernels) is the same exact result
        if case.modes != "pre":
            _setenv(monkeypatch, dict(env, **W.OFF_ENV))
            status, y, _ = L.launch(W.PLAIN, None, f"{_row_id(row)}: Winograd off")
            _lib.check(status, "Winograd off")
            W.check(f"{_row_id(row)}: Winograd off", y, W.reference(g, direction, kind, form, W.PLAIN)["y"], None, "exact")
    print(f"{_row_id(row)}: {' '.join(sorted(kernels))}: worst error / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


# ---- F(4,3), F(2,3) and the direct kernels give the same bits on exact operands ------------------------------------------------------
PAIRED = [(case, direction) for case in W.CASES if len(case.variants) >= 2 and case.modes == "all" for direction in case.directions]


@pytest.mark.parametrize("case,direction", PAIRED, ids=[f"{c.name}-{d}" for c, d in PAIRED])
def test_forms_agree_on_exact_operands(case, direction, monkeypatch):
    g = W.geometry(case, direction)
    L = Launcher(g, direction, "exact")
    results = {}
    for vname, venv in case.variants + [("off", W.OFF_ENV)]:
        env = dict(W.BASE_ENV, **venv)
        _setenv(monkeypatch, env)
        assert (W.expected_instantiation(g, direction, W.PLAIN, env) is None) == (vname == "off")
        status, y, _ = L.launch(W.PLAIN, None, f"{case.name}-{direction}-{vname}")
        _lib.check(status, vname)
        results[vname] = y
    names = list(results)
    for name in names[1:]:
        assert torch.equal(results[names[0]], results[name]), f"{case.name} {direction}: {names[0]} and {name} differ"
