"""Golden f0 tracks for the fcpe estimator, from the REFERENCE's own FCPE.py on the CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_fcpe.py

``main/library/predictors/FCPE.py`` is loaded by path with ``onnxruntime``, ``torchaudio.transforms.Resample``
and ``librosa.filters.mel`` stubbed (the last returns ``rvc_amd.melbasis``'s Slaney basis: librosa is not
installed, so the basis itself is unpinned).  A synthetic checkpoint (``rvc_amd.synthetic.fcpe_checkpoint``) is
saved to a temporary ``.pt`` and run through the reference's ``FCPE(...).compute_f0`` as ``VC.get_f0_fcpe`` calls
it (convert.py:239-246), in f32, and again with the same model in f64.

Per case ``<c>``, ``fcpe.npz`` holds ``x_<c>`` (f32 samples), ``mel32_<c>`` [T][128], ``latent32_<c>`` [T][360],
``f0m32_<c>`` / ``f0m64_<c>`` (the model's f0 [p_len], before post_process), ``f0_32_<c>`` / ``f0_64_<c>``
(compute_f0's return) and ``args_<c>`` = (hop_length, p_len, threshold, f0_min, f0_max, seed, n_layers,
use_harmonic_emb); ``fcpe_f64_<c>.npz`` holds the f64 run's ``mel64`` and ``latent64`` (apart, so that no
committed file passes 1 MiB).  ``fcpe_keys.json`` lists the default checkpoint's state-dict keys and shapes as the
reference's ``CFNaiveMelPE.state_dict()`` produces them.  Arrays only.

The generator refuses to write unless every case exercises the decoder and every frame's decisions are stable
against the reference's own f32 rounding (see ``check``).
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
from rvc_amd import melbasis, synthetic  # noqa: E402

REF = "/root/reference"
THRESHOLD, F0_MIN, F0_MAX = 0.006, 50, 1100

# name -> (samples, hop_length, checkpoint keywords)
CASES = {
    "a": (24000, 160, dict(seed=2028)),
    "b": (23999, 64, dict(seed=2028)),
    "c": (8000, 160, dict(seed=2030, n_layers=2, use_harmonic_emb=True)),
}


def load_fcpe():
    ort = types.ModuleType("onnxruntime")
    ta, tat = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.transforms")
    tat.Resample = object
    ta.transforms = tat
    lib, filt = types.ModuleType("librosa"), types.ModuleType("librosa.filters")

    def mel(sr, n_fft, n_mels, fmin, fmax):
        return melbasis.mel_filterbank(sr, n_fft, n_mels, fmin, fmax, htk=False)

    filt.mel = mel
    lib.filters = filt
    sys.modules.update({"onnxruntime": ort, "torchaudio": ta, "torchaudio.transforms": tat, "librosa": lib,
                        "librosa.filters": filt})
    path = os.path.join(REF, "main", "library", "predictors", "FCPE.py")
    spec = importlib.util.spec_from_file_location("reference_fcpe", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(mod, pt, x, hop_length, dtype):
    """The reference's compute_f0 at ``dtype`` -> (mel, latent, model f0, final f0)."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the Hann window is created at the default dtype
    try:
        fc = mod.FCPE(pt, hop_length=int(hop_length), f0_min=F0_MIN, f0_max=F0_MAX, dtype=dtype, device="cpu",
                      sample_rate=16000, threshold=THRESHOLD)
        net = fc.fcpe.model.model  # CFNaiveMelPE
        seen = {}
        fwd = net.forward

        def forward(mel, *a, **k):
            out = fwd(mel, *a, **k)
            seen["mel"], seen["latent"] = mel[0].numpy().copy(), out[0].numpy().copy()
            return out

        net.forward = forward
        infer = fc.fcpe

        def call(*a, **k):
            out = infer(*a, **k)
            seen["f0m"] = out[0, :, 0].numpy().copy()
            return out

        fc.fcpe = call
        f0 = fc.compute_f0(x, p_len=x.size // 160)
    finally:
        torch.set_default_dtype(prev)
    assert seen["mel"].dtype == seen["latent"].dtype == (np.float32 if dtype == torch.float32 else np.float64)
    return seen["mel"], seen["latent"], seen["f0m"], np.asarray(f0, dtype=np.float64)


def logit(p):
    p = p.astype(np.float64)
    return np.log(p) - np.log1p(-p)


def check(name, lat32, lat64, f0m64, cent_table):
    """The conditions the tests lean on; returns a description of the first that fails, or None."""
    l32, l64 = logit(lat32), logit(lat64)
    e = np.abs(l32 - l64).max()
    srt = np.sort(l64, axis=1)
    top, gap = srt[:, -1], srt[:, -1] - srt[:, -2]
    voiced = lat64.max(axis=1) > np.float32(THRESHOLD)
    share = voiced.mean()
    bins = np.unique(lat64.argmax(axis=1)[voiced]).size
    idx = np.flatnonzero(voiced)
    interior = idx.size > 1 and (np.diff(idx) > 1).any()
    thr = logit(np.array([np.float32(THRESHOLD)]))[0]
    # the decoded f0 of every confident frame, as the local decoder gives it (f64)
    am = lat64.argmax(axis=1)
    win = np.clip(am[:, None] + np.arange(-4, 5)[None], 0, 359)
    yl = np.take_along_axis(lat64, win, axis=1)
    f0 = 10 * 2 ** ((cent_table.astype(np.float64)[win] * yl).sum(1) / yl.sum(1) / 1200)
    edge = np.minimum(np.abs(f0 / F0_MIN - 1), np.abs(f0 / F0_MAX - 1))[voiced].min()
    print(f"{name}: e={e:.3g} min gap={gap.min():.3g} min |top - thr|={np.abs(top - thr).min():.3g} "
          f"voiced={share:.2f} bins={bins} interior={interior} edge={edge:.3g}")
    if not 0.3 <= share <= 0.8:
        return f"voiced share {share:.2f}"
    if bins < 12:
        return f"{bins} distinct bins"
    if not interior:
        return "no interior unvoiced run"
    if not (gap > 16 * e).all():
        return f"top-2 gap {gap.min():.3g} <= 16 e"
    if not (np.abs(top - thr) > 16 * e).all():
        return "a confidence within 16 e of the threshold"
    if not edge > 1e-4:
        return "a decoded f0 within 1e-4 of f0_min / f0_max"
    return None


def main():
    mod = load_fcpe()
    out = {}
    work = tempfile.mkdtemp(prefix="rvc_golden_fcpe_")
    for name, (n, hop, kw) in CASES.items():
        ckpt = synthetic.fcpe_checkpoint(**kw)
        pt = os.path.join(work, f"fcpe_{name}.pt")
        torch.save(ckpt, pt)
        x = synthetic.synthetic_audio(n / 16000.0, seed=77)[:n]
        assert x.size == n and x.dtype == np.float32
        mel32, lat32, f0m32, f0_32 = run(mod, pt, x, hop, torch.float32)
        mel64, lat64, f0m64, f0_64 = run(mod, pt, x, hop, torch.float64)
        why = check(name, lat32, lat64, f0m64, ckpt["model"]["cent_table"].numpy())
        if why:
            raise SystemExit(f"case {name}: {why}: try another seed / gain (rvc_amd.synthetic.fcpe_checkpoint)")
        assert np.array_equal(f0_32 > 0, f0_64 > 0) and np.array_equal(f0m32 > 0, f0m64 > 0)
        nz = f0_64 > 0
        print(f"  mel err {np.abs(mel32 - mel64).max():.3g}  f0 rel err "
              f"{np.abs(f0_32[nz] / f0_64[nz] - 1).max():.3g}  frames {lat64.shape[0]}  p_len {f0_64.size}")
        out.update({f"x_{name}": x, f"mel32_{name}": mel32, f"latent32_{name}": lat32,
                    f"f0m32_{name}": f0m32, f"f0m64_{name}": f0m64, f"f0_32_{name}": f0_32, f"f0_64_{name}": f0_64,
                    f"args_{name}": np.array([hop, n // 160, THRESHOLD, F0_MIN, F0_MAX, kw["seed"],
                                              kw.get("n_layers", 6), int(kw.get("use_harmonic_emb", False))])})
        np.savez_compressed(os.path.join(HERE, f"fcpe_f64_{name}.npz"), mel64=mel64, latent64=lat64)
    # the default checkpoint's keys as the reference's own module names them
    cfg = synthetic.fcpe_checkpoint()["config_dict"]["model"]
    net = mod.CFNaiveMelPE(input_channels=128, out_dims=360, hidden_dims=cfg["hidden_dims"],
                           n_layers=cfg["n_layers"], n_heads=8, f0_max=cfg["f0_max"], f0_min=cfg["f0_min"],
                           use_fa_norm=False, conv_only=True)
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "fcpe_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "fcpe.npz"), **out)


if __name__ == "__main__":
    main()
