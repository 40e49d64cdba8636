"""Golden f0 tracks for the fcpe-legacy estimator, from the REFERENCE's own FCPE.py on the CPU.

Run where ``make_golden_fcpe.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_fcpe_legacy.py

``main/library/predictors/FCPE.py`` is loaded by path with the stubs of ``make_golden_fcpe.py``.  A synthetic
checkpoint (``rvc_amd.synthetic.fcpe_legacy_checkpoint``) is saved to a temporary ``.pt`` and run through
``FCPE(pt, hop_length, f0_min=50, f0_max=1100, threshold=0.03, legacy=True).compute_f0(x, p_len=n // 160)`` as
``VC.get_f0_fcpe(legacy=True)`` calls it (convert.py:239-246), in f32, and again with the same weights in f64 (the
reference's ``STFT`` keeps its mel basis in f32 whatever the dtype, which torch's matmul refuses against an f64
spectrum: the f64 run hands it the same basis widened to f64).

Per case ``<c>``, ``fcpe_legacy.npz`` holds ``x_<c>`` (f32 samples), ``latent32_<c>`` [T][360], ``f0m32_<c>`` /
``f0m64_<c>`` (the model's f0 [p_len], before post_process), ``f0_32_<c>`` / ``f0_64_<c>`` (compute_f0's return) and
``args_<c>`` = (hop_length, p_len, threshold, seed, n_layers, out_bias); ``fcpe_legacy_f64_<c>.npz`` holds the f64 run's
``latent64`` (apart, so that no committed file passes 1 MiB).  ``fcpe_legacy_attn.npz`` pins one layer's attention on
its own, from the short case: ``x`` f32 [T][512], the input of layer 0's ``SelfAttention`` in the f32 run (``pre``:
that layer's input, before its LayerNorm), ``out32`` that module's output there, and ``out64`` the f64 model's same
module on ``x`` widened.  ``fcpe_legacy_keys.json``
lists the default checkpoint's state-dict keys and shapes as the reference's ``FCPE_LEGACY.state_dict()`` produces
them.  Arrays and names only.

The generator refuses to write unless the tests' conditions hold on the reference alone (see ``check``).  The
deepest case that passes is ``a`` / ``b``: DEEP_LAYERS layers.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_fcpe import load_fcpe, logit  # noqa: E402  (puts rvc-maker_amd on the path)
from rvc_amd import melbasis, synthetic  # noqa: E402

THRESHOLD, F0_MIN, F0_MAX = 0.03, 50, 1100
DEEP_LAYERS = 12

# name -> (samples, hop_length, checkpoint keywords); the output bias is nudged per case until no frame's confidence
# lies within 16 e of the threshold
CASES = {
    "a": (24000, 160, dict(seed=3031, n_layers=DEEP_LAYERS, out_bias=-12.7)),
    "b": (23999, 64, dict(seed=3031, n_layers=DEEP_LAYERS, out_bias=-12.9)),
    "c": (8000, 160, dict(seed=3033, n_layers=2, out_bias=-12.8)),
}


def wav2mel_at(mod, dtype):
    """The reference's Wav2Mel with its STFT's mel basis cached at ``dtype`` (see the module docstring)."""
    basis = torch.from_numpy(melbasis.mel_filterbank(16000, 1024, 128, 0, 8000, htk=False)).float().to(dtype)

    class Wav2MelAt(mod.Wav2Mel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.stft.mel_basis["8000_cpu"] = basis

    return Wav2MelAt


def run(mod, pt, x, hop_length, dtype, no_attention=False):
    """The reference's compute_f0 at ``dtype`` -> (latent, model f0, final f0, layer 0's (input, attention input),
    its attention output, the model)."""
    prev, w2m = torch.get_default_dtype(), mod.Wav2Mel
    torch.set_default_dtype(dtype)  # the Hann window is created at the default dtype
    mod.Wav2Mel = wav2mel_at(mod, dtype) if dtype == torch.float64 else w2m
    try:
        fc = mod.FCPE(pt, hop_length=int(hop_length), f0_min=F0_MIN, f0_max=F0_MAX, dtype=dtype, device="cpu",
                      sample_rate=16000, threshold=THRESHOLD, legacy=True)
        net = fc.fcpe.model  # FCPE_LEGACY
        if no_attention:
            with torch.no_grad():
                for layer in net.decoder._layers:
                    layer.attn.to_out.weight.zero_()
                    layer.attn.to_out.bias.zero_()
        seen = {}
        hooks = [net.dense_out.register_forward_hook(
                     lambda m, i, o: seen.__setitem__("latent", torch.sigmoid(o)[0].numpy().copy())),
                 net.decoder._layers[0].attn.register_forward_hook(
                     lambda m, i, o: seen.update(attn_in=i[0][0].numpy().copy(), attn_out=o[0].numpy().copy())),
                 net.decoder._layers[0].norm.register_forward_hook(
                     lambda m, i, o: seen.__setitem__("pre", i[0][0].numpy().copy()))]
        fwd = net.forward

        def forward(*a, **k):
            out = fwd(*a, **k)
            seen["f0m"] = out[0, :, 0].numpy().copy()
            return out

        net.forward = forward
        f0 = fc.compute_f0(x, p_len=x.size // 160)
        for h in hooks:
            h.remove()
    finally:
        torch.set_default_dtype(prev)
        mod.Wav2Mel = w2m
    assert seen["latent"].dtype == (np.float32 if dtype == torch.float32 else np.float64)
    return (seen["latent"], seen["f0m"], np.asarray(f0, dtype=np.float64),
            (seen["pre"], seen["attn_in"]), seen["attn_out"], net)


def decoded(lat64, cent_table):
    """The f0 of every frame as the local decoder gives it (f64)."""
    am = lat64.argmax(axis=1)
    win = np.clip(am[:, None] + np.arange(-4, 5)[None], 0, 359)
    yl = np.take_along_axis(lat64, win, axis=1)
    return 10 * 2 ** ((cent_table.astype(np.float64)[win] * yl).sum(1) / yl.sum(1) / 1200)


def check(name, lat32, lat64, lat_noattn, cent_table):
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
    moved = (lat_noattn.argmax(axis=1) != lat64.argmax(axis=1)).mean()
    f0 = decoded(lat64, cent_table)
    outside = int(((f0 < F0_MIN) | (f0 > F0_MAX))[voiced].sum())
    print(f"{name}: e={e:.3g} (16 e={16 * e:.3g}) min gap={gap.min():.3g} "
          f"min |top - thr|={np.abs(top - thr).min():.3g} voiced={share:.2f} bins={bins} interior={interior} argmax moved without attention={moved:.2f} "
          f"voiced frames outside {F0_MIN}..{F0_MAX} Hz={outside}")
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
    if not moved >= 0.25:
        return f"the attention decides only {moved:.2f} of the frames"
    return None


def main():
    mod = load_fcpe()
    out, attn = {}, None
    work = tempfile.mkdtemp(prefix="rvc_golden_fcpe_legacy_")
    for name, (n, hop, kw) in CASES.items():
        ckpt = synthetic.fcpe_legacy_checkpoint(**kw)
        pt = os.path.join(work, f"fcpe_legacy_{name}.pt")
        torch.save(ckpt, pt)
        x = synthetic.synthetic_audio(n / 16000.0, seed=77)[:n]
        assert x.size == n and x.dtype == np.float32
        lat32, f0m32, f0_32, (pre, ain), aout32, _ = run(mod, pt, x, hop, torch.float32)
        lat64, f0m64, f0_64, _, _, net64 = run(mod, pt, x, hop, torch.float64)
        lat_na = run(mod, pt, x, hop, torch.float64, no_attention=True)[0]
        why = check(name, lat32, lat64, lat_na, ckpt["model"]["cent_table"].numpy())
        if why:
            raise SystemExit(f"case {name}: {why}: try another seed / gain "
                             "(rvc_amd.synthetic.fcpe_legacy_checkpoint)")
        assert np.array_equal(f0_32 > 0, f0_64 > 0) and np.array_equal(f0m32 > 0, f0m64 > 0)
        nz = f0_64 > 0
        print(f"  f0 rel err {np.abs(f0_32[nz] / f0_64[nz] - 1).max():.3g}  frames {lat64.shape[0]}  "
              f"p_len {f0_64.size}  f0m range {f0m64[f0m64 > 0].min():.1f}..{f0m64.max():.1f}")
        out.update({f"x_{name}": x, f"latent32_{name}": lat32, f"f0m32_{name}": f0m32, f"f0m64_{name}": f0m64,
                    f"f0_32_{name}": f0_32, f"f0_64_{name}": f0_64,
                    f"args_{name}": np.array([hop, n // 160, THRESHOLD, kw["seed"], kw["n_layers"], kw["out_bias"]])})
        np.savez_compressed(os.path.join(HERE, f"fcpe_legacy_f64_{name}.npz"), latent64=lat64)
        if name == "c":
            with torch.no_grad():
                aout64 = net64.decoder._layers[0].attn(torch.from_numpy(ain).double()[None])[0].numpy()
            assert ain.dtype == aout32.dtype == np.float32 and ain.shape == (n // 160 + 1, 512)
            print(f"  attention: T={ain.shape[0]} |x| rms {np.sqrt((ain ** 2).mean()):.3g} "
                  f"max |out32 - out64| {np.abs(aout32 - aout64).max():.3g} max |out64| {np.abs(aout64).max():.3g}")
            attn = dict(pre=pre, x=ain, out32=aout32, out64=aout64,
                        args=np.array([kw["seed"], kw["n_layers"], kw["out_bias"]]))
    # the default checkpoint's keys as the reference's own module names them
    cfg = synthetic.fcpe_legacy_checkpoint()["config"]["model"]
    net = mod.FCPE_LEGACY(input_channel=128, out_dims=360, n_layers=cfg["n_layers"], n_chans=cfg["n_chans"])
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "fcpe_legacy_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "fcpe_legacy_attn.npz"), **attn)
    np.savez_compressed(os.path.join(HERE, "fcpe_legacy.npz"), **out)


if __name__ == "__main__":
    main()
