"""bench.py end to end on the device: a plain run prints the headline line without the --full legs in every --input mode,
--full adds them, and --dump-outputs writes the same arrays for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "cpu_baseline", "phases", "extra", "resident_input_same_process")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["resident", "u8"])
def test_plain_run_prints_the_headline_without_the_full_legs(mode, tmp_path):
    runs = [_bench("--input", mode, "--dump-outputs", str(tmp_path / name)) for name in ("a", "b")]
    for d in runs:
        assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "clips/s" and d["dtype"] == "f32"
        assert not [k for k in FULL_ONLY if k in d] and "idle_queue" not in d["host_enqueue_ms"]
        assert d["config"]["input"] == mode and (("pcie_bytes_per_step" in d["config"]) == (mode == "u8"))
    names = sorted(runs[0]["outputs_dumped"]["arrays"])
    assert names == ["embeddings", "loss", "state_sample", "state_sample_index"]
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a))
        assert np.array_equal(a, b), n                       # same arguments: same inputs, same step


@pytest.mark.gpu
def test_full_u8_run_adds_the_resident_reference():
    d = _bench("--input", "u8", "--full", "--no-cpu-baseline")
    assert d["full"] is True and "roofline" in d and "idle_queue" in d["host_enqueue_ms"]
    assert d["resident_input_same_process"]["unit"] == "clips/s" and d["resident_input_same_process"]["ms_per_step"] > 0
