#!/usr/bin/env python3
"""Records tests/golden/wgrad_host_answers.json: the host-side answers of the weight-gradient entry points (workspace and mask
sizes, prologue support, refusals) for every (row, switch set) pair of tests/wgrad_cases.py.  Needs the built library and no GPU:
every call returns before anything is launched.  Run it when a tuning change is MEANT to move a slice count or a route, never
to make tests/test_wgrad_host.py pass.

    python tools/make_wgrad_host_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import wgrad_cases as W  # noqa: E402
import test_ops_gpu as T  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ops  # noqa: E402

E_WORKSPACE, E_UNSUPPORTED = 3, 6               # include/zsv_hip.h


def main():
    lib = _lib.load()
    stale = [k for k in os.environ if k.startswith("ZSV_") and k != "ZSV_LIB_PATH"]
    if stale:
        raise SystemExit(f"unset {stale} first: the answers depend on the switches")
    out = {}
    for switches in W.SWITCH_SETS:
        os.environ.update(switches)
        _lib.reload_knobs()
        for row in W.rows(T.WGRAD_DMA_CASES, T.WGRAD_WINO_CASES, T.WGRAD_TRING_CASES):
            a = W.answers(lib, ops.conv_desc(row.xs, row.ws, row.stride, row.padding))
            short = a["short_workspace"]
            if short is not None and not (short[0] == short[1] == E_WORKSPACE and short[2] in (E_WORKSPACE, E_UNSUPPORTED)):
                raise SystemExit(f"{row.name} {switches}: a workspace one byte short was not refused ({short})")
            out[f"{row.name} {W.switch_id(switches)}"] = a
        for k in switches:
            del os.environ[k]
        _lib.reload_knobs()
    path = os.path.join(ROOT, "tests", "golden", "wgrad_host_answers.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{len(out)} answers -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
