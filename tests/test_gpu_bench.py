"""bench.py end to end at a short clip: every leg of a --full run (clip stream, per-call pass, roofline probe) must
run on the current tree and print one well-formed contract line, and --dump-outputs must hand over the last timed
step's waveforms."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_short_clip(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--seconds", "4", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] > 0 and line["n_gpus"] == 1 and line["steps"] == 2
    roof = line["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and roof["launches_per_step"] > 0
    assert line["per_call"]["value"] > 0
    # the last timed step's waveform: one clip per step, peak-normalised, of the length the line states
    assert sorted(os.listdir(dump)) == ["waveform_0.npy"]
    w = np.load(dump / "waveform_0.npy")
    assert w.dtype == np.float32 and w.shape == (round(line["config"]["output_seconds_per_clip"] * 48000),)
    assert np.isfinite(w).all() and 0 < np.abs(w).max() <= 1.0


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """dump_outputs writes float32 files; beyond the byte limit, a fixed sample of each waveform's positions that
    fits the limit and is the same from call to call."""
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    waves = [torch.arange(1000, dtype=torch.float64), torch.arange(500, dtype=torch.float32) * 0.5]
    bench.dump_outputs(str(tmp_path / "a"), waves)
    a = [np.load(tmp_path / "a" / f"waveform_{i}.npy") for i in range(2)]
    assert all(x.dtype == np.float32 for x in a)
    np.testing.assert_array_equal(a[0], np.arange(1000, dtype=np.float32))
    np.testing.assert_array_equal(a[1], np.arange(500, dtype=np.float32) * 0.5)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3000)  # the two waveforms hold 6000 bytes as float32
    bench.dump_outputs(str(tmp_path / "b"), waves)
    bench.dump_outputs(str(tmp_path / "c"), waves)
    b = [np.load(tmp_path / "b" / f"waveform_{i}.npy") for i in range(2)]
    c = [np.load(tmp_path / "c" / f"waveform_{i}.npy") for i in range(2)]
    assert sum(x.nbytes for x in b) <= 3000 and [x.size for x in b] == [500, 250]
    for x, y, full in zip(b, c, a):
        np.testing.assert_array_equal(x, y)
        assert np.all(np.diff(x) > 0) and np.isin(x, full).all()  # distinct samples of the waveform, in order
