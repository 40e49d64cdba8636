"""Golden f0 tracks for the swipe estimator, from the REFERENCE's own SWIPE.py on the CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_swipe.py

``main/library/predictors/SWIPE.py`` is loaded by path and called as ``VC.get_f0_swipe`` calls it
(convert.py:272-276: ``swipe(x.astype(np.float32), 16000, f0_floor=50, f0_ceil=1100, frame_period=10)``).
``swipe.npz`` holds, per input, ``x_<name>`` (the f32 samples) and ``f0_<name>`` (the reference's f32 f0):
arrays only.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

from make_golden import OUT, REF, synthetic


def load_swipe():
    path = os.path.join(REF, "main", "library", "predictors", "SWIPE.py")
    spec = importlib.util.spec_from_file_location("reference_swipe", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.swipe


def vibrato(seconds=1.5, f=150.0, depth=0.1, rate=1.5, lead=0.5, tail=0.25, sr=16000):
    """The vibrato of tests/test_gpu_pm.py."""
    t = np.arange(int(seconds * sr)) / sr
    ph = 2 * np.pi * np.cumsum(f * (1 + depth * np.sin(2 * np.pi * rate * t))) / sr
    x = 0.5 * np.sin(ph) + 0.2 * np.sin(2 * ph) + 0.1 * np.sin(3 * ph)
    x = np.concatenate([np.zeros(int(lead * sr)), x, np.zeros(int(tail * sr))])
    return x + 1e-4 * np.random.default_rng(0).standard_normal(len(x))


def sweep(seconds=2.2, sr=16000):
    """A harmonic sweep 70 Hz * 2^(3.8 t / 2.2): eight harmonics, each while below 7.6 kHz, 1e-3 noise."""
    t = np.arange(int(seconds * sr)) / sr
    f = 70.0 * 2 ** (3.8 * t / seconds)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = np.zeros_like(t)
    for h in range(1, 9):
        x += np.where(h * f < 7600.0, np.sin(h * ph) / h, 0.0)
    return 0.3 * x + 1e-3 * np.random.default_rng(7).standard_normal(len(t))


def inputs():
    speech = synthetic.synthetic_audio(3.0, seed=31)
    sig = {"vibrato": vibrato(), "speechlike": speech,
           "noise": 0.3 * np.random.default_rng(5).standard_normal(16000), "silence": np.zeros(8000),
           "sweep": sweep()}
    for n in (161, 700, 2049, 16037):
        sig[f"slice{n}"] = speech[8000:8000 + n]
    return {k: np.asarray(v).astype(np.float32) for k, v in sig.items()}


def main():
    swipe = load_swipe()
    out = {}
    for name, x in inputs().items():
        f0, _ = swipe(x.astype(np.float32), 16000, f0_floor=50, f0_ceil=1100, frame_period=10)
        assert f0.dtype == np.float32 and len(f0) == len(x) // 160 + 1
        out["x_" + name], out["f0_" + name] = x, f0
        print(name, len(x), int((f0 > 0).sum()), "voiced of", len(f0))
    np.savez_compressed(os.path.join(OUT, "swipe.npz"), **out)


if __name__ == "__main__":
    main()
