"""Weight-gradient geometries and switch sets whose host-side answers are pinned (TEST INFRASTRUCTURE; never imported by the
package, no GPU import).

Which kernel serves a weight gradient, how many slices it cuts the voxel range into and how much workspace that takes are all
decided on the host (conv_wgrad.hip's route table, wgrad_plan.h).  ``tests/test_wgrad_host.py`` asks the library's queries and
its refusals for every (row, switch set) pair below and compares them with ``tests/golden/wgrad_host_answers.json``, which
``tools/make_wgrad_host_golden.py`` recorded; nothing is launched and nothing dereferenced, so no GPU is needed.  A tuning
change that moves a slice count regenerates the file on purpose.
"""
from collections import namedtuple

WgradRow = namedtuple("WgradRow", "name xs ws stride padding")

SWITCH_SETS = [
    {},
    {"ZSV_NO_WGRAD_WINO": "1"}, {"ZSV_NO_WGRAD_WINO4": "1"}, {"ZSV_NO_WGRAD_TRING": "1"}, {"ZSV_NO_WGRAD_TWINO": "1"},
    {"ZSV_NO_WGRAD_DMA": "1"}, {"ZSV_NO_T2_DENSE": "1"}, {"ZSV_NO_STEM_WGRAD": "1"},
    {"ZSV_WGRAD_TRING_SLICES": "7"}, {"ZSV_WGRAD_WINO_SLICES": "9"}, {"ZSV_WGRAD_DMA_SLICES": "25"}, {"ZSV_WGRAD_CFG": "2"},
    {"ZSV_WGRAD_BN": "64"},
]


def switch_id(switches):
    return ",".join(f"{k}={v}" for k, v in switches.items()) or "default"


BATCH, FRAMES, SIZE = 22, 16, 112             # bench.py: clips per GPU, frames per clip, frame size


def _out(v, k, s, p):
    return (v + 2 * p - k) // s + 1


def _add(rows, name, n, cin, thw, cout, k, s, p):
    rows.append(WgradRow(name, (n, cin) + tuple(thw), (cout, cin) + tuple(k), tuple(s), tuple(p)))
    return tuple(_out(v, kk, ss, pp) for v, kk, ss, pp in zip(thw, k, s, p))


def _midplanes(inplanes, planes):
    return (inplanes * planes * 3 * 3 * 3) // (inplanes * 3 * 3 + 3 * planes)


def resnet18_rows(factorised):
    """Every convolution of R(2+1)D-18 (factorised) or R3D-18 on BATCH clips of FRAMES x SIZE x SIZE."""
    rows, who = [], "r2plus1d" if factorised else "r3d"
    thw = (FRAMES, SIZE, SIZE)
    if factorised:
        thw = _add(rows, f"{who}_stem_s", BATCH, 3, thw, 45, (1, 7, 7), (1, 2, 2), (0, 3, 3))
        thw = _add(rows, f"{who}_stem_t", BATCH, 45, thw, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    else:
        thw = _add(rows, f"{who}_stem", BATCH, 3, thw, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3))
    inplanes = 64
    for layer, planes in enumerate((64, 128, 256, 512), start=1):
        for block in range(2):
            stride = 2 if layer > 1 and block == 0 else 1
            mid = _midplanes(inplanes, planes)
            if stride == 2:
                _add(rows, f"{who}_l{layer}_down", BATCH, inplanes, thw, planes, (1, 1, 1), (2, 2, 2), (0, 0, 0))
            for conv, (cin, s) in enumerate(((inplanes, stride), (planes, 1)), start=1):
                tag = f"{who}_l{layer}b{block}c{conv}"
                if factorised:
                    thw = _add(rows, tag + "s", BATCH, cin, thw, mid, (1, 3, 3), (1, s, s), (0, 1, 1))
                    thw = _add(rows, tag + "t", BATCH, mid, thw, planes, (3, 1, 1), (s, 1, 1), (1, 0, 0))
                else:
                    thw = _add(rows, tag, BATCH, cin, thw, planes, (3, 3, 3), (s, s, s), (1, 1, 1))
            inplanes = planes
    return rows


def c3d_rows():
    rows, thw = [], (FRAMES, SIZE, SIZE)
    plan = [("conv1", 3, 64, (1, 2, 2)), ("conv2", 64, 128, (2, 2, 2)), ("conv3a", 128, 256, None), ("conv3b", 256, 256, (2, 2, 2)),
            ("conv4a", 256, 512, None), ("conv4b", 512, 512, (2, 2, 2)), ("conv5a", 512, 512, None), ("conv5b", 512, 512, None)]
    for name, cin, cout, pool in plan:
        thw = _add(rows, f"c3d_{name}", BATCH, cin, thw, cout, (3, 3, 3), (1, 1, 1), (1, 1, 1))
        if pool:
            thw = tuple(v // p for v, p in zip(thw, pool))
    return rows


EXTRA = [
    WgradRow("stem_small", (2, 3, 4, 32, 32), (45, 3, 1, 7, 7), (1, 2, 2), (0, 3, 3)),
    WgradRow("cin_5_full_333", (2, 5, 4, 9, 9), (12, 5, 3, 3, 3), (1, 1, 1), (1, 1, 1)),                  # Cin < 16: generic kernel
    WgradRow("two_frames_temporal", (3, 288, 2, 7, 7), (128, 288, 3, 1, 1), (1, 1, 1), (1, 0, 0)),       # t2-dense fold
    WgradRow("spatial_stride2", (2, 16, 2, 14, 14), (45, 16, 1, 3, 3), (1, 2, 2), (0, 1, 1)),            # staged kernel only
]


X_ADDR, DY_ADDR, DW_ADDR, COEF_ADDR, WS_ADDR = 0x10000, 0x7f0000, 0xa00000, 0xb00000, 0x1000000    # never dereferenced, 16-byte aligned


def answers(lib, d):
    """The host-side answers of one geometry under the current switches, as JSON-ready values.  Every call here returns before
    anything is launched or dereferenced: the operands are made-up addresses."""
    from ctypes import byref
    need = int(lib.zsv_conv3d_wgrad_workspace_bytes(byref(d)))
    a = {"workspace_bytes": need,
         "mask_bytes": int(lib.zsv_conv3d_wgrad_mask_bytes(byref(d))),
         "pre_supported": int(lib.zsv_conv3d_pre_supported(byref(d))),
         "mask_null_table": int(lib.zsv_conv3d_wgrad_mask(byref(d), None, None))}
    operands = [X_ADDR, DY_ADDR, DW_ADDR]
    for i, missing in enumerate(("x", "dy", "dw")):
        ops = [None if j == i else v for j, v in enumerate(operands)]
        x, dy, dw = ops
        a[f"null_{missing}"] = [int(lib.zsv_conv3d_wgrad(byref(d), x, dy, dw, WS_ADDR, need, None)),
                                int(lib.zsv_conv3d_wgrad_masked(byref(d), x, dy, dw, WS_ADDR, need, None, None)),
                                int(lib.zsv_conv3d_wgrad_pre(byref(d), x, COEF_ADDR, d.Cin, dy, dw, WS_ADDR, need, None))]
    a["null_coef"] = int(lib.zsv_conv3d_wgrad_pre(byref(d), X_ADDR, None, d.Cin, DY_ADDR, DW_ADDR, WS_ADDR, need, None))
    # one byte short (a geometry that needs no workspace cannot be one byte short: nothing is asked)
    a["short_workspace"] = None if need == 0 else [
        int(lib.zsv_conv3d_wgrad(byref(d), X_ADDR, DY_ADDR, DW_ADDR, WS_ADDR, need - 1, None)),
        int(lib.zsv_conv3d_wgrad_masked(byref(d), X_ADDR, DY_ADDR, DW_ADDR, WS_ADDR, need - 1, None, None)),
        int(lib.zsv_conv3d_wgrad_pre(byref(d), X_ADDR, COEF_ADDR, d.Cin, DY_ADDR, DW_ADDR, WS_ADDR, need - 1, None))]
    return a


def rows(dma_cases, wino_cases, tring_cases):
    """test_ops_gpu's three weight-gradient case lists, the small rows above, then the three networks' layers (each geometry once)."""
    out = []
    for name, n, cin, thw, cout, k, p in dma_cases:
        out.append(WgradRow(f"dma/{name}", (n, cin) + thw, (cout, cin) + k, (1, 1, 1), p))
    for name, n, cin, thw, cout, kt in wino_cases:
        out.append(WgradRow(f"wino/{name}", (n, cin) + thw, (cout, cin, kt, 3, 3), (1, 1, 1), (kt // 2, 1, 1)))
    for name, n, cin, thw, cout in tring_cases:
        out.append(WgradRow(f"tring/{name}", (n, cin) + thw, (cout, cin, 3, 1, 1), (1, 1, 1), (1, 0, 0)))
    out += EXTRA
    seen = set()
    for r in resnet18_rows(True) + resnet18_rows(False) + c3d_rows():
        if r[1:] not in seen:
            seen.add(r[1:])
            out.append(r)
    return out
