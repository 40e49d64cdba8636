"""Recorded outputs of every f0 route of the conversion and extraction paths, from the project's own code on the GPU.

    python tests/golden/make_golden_f0_paths.py [OUT]      # writes tests/golden/f0_paths.npz (or OUT)

The file pins behaviour across refactors of the f0 plumbing: it was written at the commit before ``rvc_amd/f0.py``
existed, and tests/test_gpu_f0_paths.py reproduces every case bit for bit.  Only entry points that are the same
before and after are used -- ``VC.f0_device`` and ``FeatureInputAMD.compute_f0`` -- so the script regenerates the
file at either commit.

One signal, ``synthetic_audio`` cut to 12 040 samples: p_len = 75 and 76 estimator frames (RMVPE pads to 96), a
Praat track shorter than p_len (pm's zero padding on both sides), a length that is no multiple of 160.  Synthetic
weights: rmvpe, crepe-tiny with its dither fixed to the stored draw ``dither``, a one-layer 64-channel fcpe and
fcpe-legacy.  The conversion-side VC has x_pad = 0, so that the f0 file's frames start at frame 0 of this short
track (the signal stands for the unpadded one).

Cases ``vc:<method>:<variant>`` hold ``:coarse`` (int64) and ``:pitchf`` (f32): every single method and three
hybrids, each plain (pitch 0), with pitch +3 and autotune 0.5, and with pitch -2 and an f0 file over frames 0..40.
Cases ``fi:<method>:<hop>`` hold ``:f0``, compute_f0's return.  ``<case>:voiced`` is the count of non-zero frames.

Every case runs twice; the script refuses to write one whose two runs differ in any bit, or whose track has fewer
than MIN_VOICED non-zero frames (an all-unvoiced track would hide a wrong shift or override).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "rvc-maker_amd"))
from rvc_amd import synthetic  # noqa: E402

DEV = "cuda"
N, P_LEN, MIN_VOICED = 12040, 75, 10
AUDIO_SEED = 31
SEEDS = {"rmvpe": 9, "crepe": 1240, "fcpe": 2028, "fcpe_legacy": 3033}
FCPE_LEGACY_OUT_BIAS = -12.8
SINGLE = ("rmvpe", "crepe-tiny", "pm", "swipe", "fcpe", "fcpe-legacy")
HYBRIDS = ("hybrid[pm+swipe+fcpe]", "hybrid[rmvpe+crepe-tiny+fcpe-legacy]", "hybrid[swipe+swipe]")
F0_FILE = np.array([[0.00, 110.0], [0.15, 220.0], [0.25, 0.0], [0.40, 330.0]], np.float32)
# variant -> (pitch, autotune, strength, f0 file)
VARIANTS = {"plain": (0, False, 1.0, None), "tune": (3, True, 0.5, None), "file": (-2, False, 1.0, F0_FILE)}
EXTRACT = [(m, 160) for m in ("rmvpe", "crepe-tiny", "swipe", "fcpe", "fcpe-legacy")] + \
          [("hybrid[pm+rmvpe+fcpe]", 64), ("hybrid[pm+rmvpe+fcpe]", 160)]


def signal():
    return synthetic.synthetic_audio(1.0, seed=AUDIO_SEED)[:N].astype(np.float32)


def draw_dither():
    return np.random.default_rng(3).triangular(-20, 0, 20, size=128)


def case_names():
    return [f"vc:{m}:{v}" for m in SINGLE + HYBRIDS for v in VARIANTS] + [f"fi:{m}:{h}" for m, h in EXTRACT]


class Paths:
    """The two owners of the estimators, on one set of synthetic models."""

    def __init__(self, dither):
        from rvc_amd.crepe import CrepeAMD
        from rvc_amd.extract import FeatureInputAMD
        from rvc_amd.fcpe import FcpeAMD
        from rvc_amd.fcpe_legacy import FcpeLegacyAMD
        from rvc_amd.pipeline import VC, Config
        from rvc_amd.rmvpe import RMVPEAMD
        kw = dict(rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(SEEDS["rmvpe"]), DEV),
                  crepe={"tiny": CrepeAMD(synthetic.crepe_state_dict(SEEDS["crepe"], "tiny"), "tiny", DEV)},
                  fcpe=FcpeAMD(synthetic.fcpe_checkpoint(SEEDS["fcpe"], n_layers=1, hidden_dims=64), DEV),
                  fcpe_legacy=FcpeLegacyAMD(synthetic.fcpe_legacy_checkpoint(
                      SEEDS["fcpe_legacy"], n_layers=1, n_chans=64, out_bias=FCPE_LEGACY_OUT_BIAS), DEV))
        kw["crepe"]["tiny"].dither_fn = lambda T: dither[:T]
        cfg = Config(DEV)
        cfg.x_pad = 0
        self.vc = VC(40000, cfg, **kw)
        self.fi = FeatureInputAMD(device=DEV, **kw)
        self.x = signal()
        self.xp = torch.from_numpy(self.x).to(DEV)
        self.xp64 = self.xp.double()

    def run(self, name):
        """-> {suffix: array} of one case."""
        owner, method, arg = name.split(":")
        if owner == "vc":
            pitch, autotune, strength, f0_file = VARIANTS[arg]
            coarse, pitchf = self.vc.f0_device(self.xp, pitch, method, autotune, strength, f0_file, xp64=self.xp64)
            out = {"coarse": coarse.cpu().numpy(), "pitchf": pitchf.cpu().numpy()}
        else:
            out = {"f0": np.asarray(self.fi.compute_f0(self.x, method, int(arg)))}
        self.vc.check_errors()
        return out


def track(out):
    return out["pitchf"] if "pitchf" in out else out["f0"]


def main():
    dither = draw_dither()
    paths = Paths(dither)
    data, bad = {"dither": dither, "x": paths.x}, []
    for name in case_names():
        first, second = paths.run(name), paths.run(name)
        voiced = int(np.count_nonzero(track(first)))
        same = all(first[k].dtype == second[k].dtype and first[k].shape == second[k].shape and
                   first[k].tobytes() == second[k].tobytes() for k in first)
        print(f"{name}: {', '.join(f'{k} {v.dtype} {v.shape}' for k, v in first.items())}; voiced {voiced} of "
              f"{track(first).size}{'' if same else '; TWO RUNS DIFFER'}", flush=True)
        if not same or voiced < MIN_VOICED:
            bad.append(name)
        for k, v in first.items():
            data[f"{name}:{k}"] = v
        data[f"{name}:voiced"] = np.int64(voiced)
    if bad:
        raise SystemExit(f"not written: {bad} (two runs differ, or fewer than {MIN_VOICED} voiced frames)")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f0_paths.npz")
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {len(case_names())} cases")


if __name__ == "__main__":
    main()
