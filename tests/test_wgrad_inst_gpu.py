"""Every instantiation of the specialised fp32 weight-gradient kernels (csrc/conv_wgrad_wino.hip, conv_wgrad_tring.hip,
conv_wgrad_generic.hip, t2_fold_kernel of conv_wgrad.hip), forced on the smallest shapes its route admits, against an fp64
reference: bit for bit on exactly representable operands (the F(4,3) form within the rounding of its output transform), within a
derived per-element bound on standard-normal ones (tests/wgrad_inst_cases.py: rows, restated planners, operands, references, bounds).

Every launch goes through the C ABI (zsv_conv3d_wgrad, zsv_conv3d_wgrad_pre, zsv_conv3d_wgrad_masked with a table from
zsv_conv3d_wgrad_mask) under exactly the row's switches, with dw and a workspace of exactly the queried size between NaN-filled guard
bands.  Per run: the comparison, one repeat (bitwise reproducible), the masked call (same bits) on the rows that take a table, and in
the ``exact`` kind the forced slice counts 1 and 7 (same bits as the planner's own count), the prologue call against the plain call
on the materialised relu(x * scale + shift) (same bits) and the name of the kernel that ran, read from a kernel trace.  The trace's
names carry the template arguments as the demangler prints them; they are compared with ``expected_instantiation`` when they are
there, and the kernel family alone when a trace has none (the arguments are then left to the host test's planner check).  Every test
prints the kernel it reached and its worst error / bound ratio (0 where the comparison is ``torch.equal``).
"""
import ctypes
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_inst_cases as G  # noqa: E402
from guarded import guarded, guarded_like  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ops  # noqa: E402

DEV = "cuda"


def _setenv(monkeypatch, env):
    """Exactly ``env`` of the matrix's switches: the others are unset (a forced slice count left over from the launch before would
    turn every later launch into that count)."""
    for name in G.switch_names() - set(env):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _dev(t):
    return t.float().contiguous().to(DEV)


class Launcher:
    """The device operands of one (geometry, kind) and the three entry points on them."""

    def __init__(self, g, kind, pre):
        self.g, self.lib = g, _lib.load()
        self.d = ops.conv_desc(g.xs, (g.cout, g.xs[1]) + g.kernel, g.stride, g.padding)
        x, _, _, _, dy = G.operands(g, kind, amp=G.AMP)
        self.x, self.dy = _dev(x), _dev(dy)
        self.coef = _dev(G.pre_coef(g, kind)[2]) if pre else None
        self.act = _dev(G.activation(g, kind)[0]) if pre and kind == "exact" else None
        self.wshape = (g.cout, g.xs[1]) + g.kernel

    def launch(self, what, pre=False, masked=False, x=None):
        """dw of one call; the guard bands of dw and of the workspace are checked."""
        lib, d = self.lib, ctypes.byref(self.d)
        x = self.x if x is None else x
        out = guarded_like(torch.float32, self.wshape, DEV, 0xFF)               # 0xFF bytes: NaN
        dw = out.view(torch.float32, self.wshape)
        nbytes = int(lib.zsv_conv3d_wgrad_workspace_bytes(d))
        ws = guarded(nbytes, DEV, 0xFF)
        bufs = [(out, "dw"), (ws, "workspace")]
        if pre:
            status = lib.zsv_conv3d_wgrad_pre(d, x.data_ptr(), self.coef.data_ptr(), self.coef.shape[1], self.dy.data_ptr(), dw.data_ptr(),
                                              ws.ptr, nbytes, None)
        elif masked:
            mbytes = int(lib.zsv_conv3d_wgrad_mask_bytes(d))
            assert mbytes > 0, f"{what}: no mask table for this shape"
            mask = guarded(mbytes, DEV, 0xFF)
            bufs.append((mask, "mask table"))
            _lib.check(lib.zsv_conv3d_wgrad_mask(d, mask.ptr, None), f"{what}: zsv_conv3d_wgrad_mask")
            status = lib.zsv_conv3d_wgrad_masked(d, x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), ws.ptr, nbytes, mask.ptr, None)
        else:
            status = lib.zsv_conv3d_wgrad(d, x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), ws.ptr, nbytes, None)
        torch.cuda.synchronize()
        _lib.check(status, what)
        for buf, name in bufs:
            buf.check(f"{what}: {name}")
        return dw.clone()


def _kernel_names(fn):
    """The names (without spaces) of the kernels ``fn`` ran on the device, from a kernel trace."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key.replace(" ", "") for e in prof.key_averages() if e.device_type == DeviceType.CUDA]


def _template_arguments(name, family):
    """The template arguments of ``family`` in a demangled kernel name as a tuple of ints (bools as 0 / 1), or None without any."""
    m = re.search(r"(?<![A-Za-z0-9_])" + family + r"<([^<>]*)>", name)
    if m is None:
        return None
    args = [a.replace("(bool)", "").replace("(int)", "") for a in m.group(1).split(",")]
    return tuple(1 if a == "true" else 0 if a == "false" else int(a) for a in args)


def _assert_kernel(what, names, inst):
    """Of the matrix's kernel families exactly the expected one ran, with the expected template arguments where the trace has them."""
    ran = {f for f in G.FAMILIES for n in names if re.search(r"(?<![A-Za-z0-9_])" + f + r"(?![A-Za-z0-9_])", n)}
    assert ran == {inst[0]}, f"{what}: expected {inst[0]}, the trace has {sorted(ran)} among {names}"
    seen = {_template_arguments(n, inst[0]) for n in names if re.search(r"(?<![A-Za-z0-9_])" + inst[0] + r"(?![A-Za-z0-9_])", n)}
    seen.discard(None)
    if inst[1] and seen:
        assert seen == {tuple(inst[1])}, f"{what}: expected {inst[0]}<{inst[1]}>, the trace has {sorted(seen)}"
    return bool(seen) or not inst[1]


CASES = [(run, kind) for run in G.runs() for kind in G.KINDS]


def _case_id(case):
    return f"{G.run_id(case[0])}-{case[1]}"


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_forced_instantiation(case, monkeypatch):
    run, kind = case
    g, env, pre, what = run.row.geom, run.env, run.pre, _case_id(case)
    _setenv(monkeypatch, env)
    inst = G.expected_instantiation(g, env, pre)
    ref = G.reference(g, kind, G.form_of(g, env, pre), pre)
    L = Launcher(g, kind, pre)
    assert int(L.lib.zsv_conv3d_wgrad_workspace_bytes(ctypes.byref(L.d))) == G.workspace_bytes(g, env), f"{what}: workspace bytes"

    dw = L.launch(what, pre=pre)
    ratio = G.compare(what, dw, ref, kind)
    assert torch.equal(dw, L.launch(f"{what}: repeat", pre=pre)), f"{what}: not bitwise reproducible"

    if G.mask_bytes(g, env):
        assert torch.equal(dw, L.launch(f"{what}: masked", masked=True)), f"{what}: the caller's mask table changes the bits"
    else:
        assert int(L.lib.zsv_conv3d_wgrad_mask_bytes(ctypes.byref(L.d))) == 0

    notes = []
    if kind == "exact":
        if run.row.slices:
            counts = [G.planned_slices(g, env)]
            for s in G.FORCED_SLICES:
                e = dict(env, **{run.row.slices: str(s)})
                _setenv(monkeypatch, e)
                counts.append(G.planned_slices(g, e))
                other = L.launch(f"{what}: {s} slice(s)", pre=pre)
                assert torch.equal(dw, other), \
                    f"{what}: {int((dw != other).sum())} elements depend on the slice count ({counts[0]} vs {counts[-1]} slices)"
            _setenv(monkeypatch, env)
            notes.append(f"slices {counts[0]} = 1 = 7")
        if pre:
            plain = L.launch(f"{what}: plain call on the materialised activation", x=L.act)
            assert torch.equal(dw, plain), f"{what}: the prologue differs from the materialised relu(x * scale + shift)"
        names = _kernel_names(lambda: L.launch(f"{what}: traced", pre=pre))
        notes.append("template arguments from the trace" if _assert_kernel(what, names, inst) else "kernel family from the trace")
    print(f"{what}: {inst[0]}<{','.join(str(v) for v in inst[1])}>: worst error / bound {ratio:.2e}" + "".join(f"; {n}" for n in notes))
