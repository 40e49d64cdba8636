"""Deterministic synthetic checkpoints and audio for the VC hot path.

No pretrained weights exist offline, so every test and the bench
use true-shape weights generated here from a seed.  The generator writes the
three checkpoint layouts the reference loads:

* voice model ``.pth``  -- ``{"weight": {k: fp16}, "config": [18 items], "f0",
  "version", "vocoder", "sr", ...}`` exactly as
  ``main/inference/train.py:729-742`` saves it (weight-norm stored as
  ``.weight_g`` / ``.weight_v``, ``enc_q`` dropped);
* embedder ``.pt``     -- fairseq ``{"cfg": {"model": HubertConfig kwargs,
  "task": {}}, "model": state_dict}`` read by
  ``main/library/architectures/fairseq.py:30-36``;
* ``rmvpe.pt``         -- a plain ``E2E(4, 1, (2, 2))`` state dict
  (``main/library/predictors/RMVPE.py:196-198``).

Values come from numpy's PCG64 so the same seed gives the same bytes on this
container and on the GPU box.  Scales are chosen so activations stay O(1)
through every stage (the reference's own init zeroes the flow's ``post`` conv,
which would make the flow an identity and hide it from parity tests).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

# main/configs/v{1,2}/{32000,40000,48000}.json ("model" + "data" sections).
_SR_TABLE = {
    32000: dict(filter_length=1024, v1=dict(upsample_rates=[10, 4, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4]),
                v2=dict(upsample_rates=[10, 8, 2, 2], upsample_kernel_sizes=[20, 16, 4, 4])),
    40000: dict(filter_length=2048, v1=dict(upsample_rates=[10, 10, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4]),
                v2=dict(upsample_rates=[10, 10, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4])),
    48000: dict(filter_length=2048, v1=dict(upsample_rates=[10, 6, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4]),
                v2=dict(upsample_rates=[12, 10, 2, 2], upsample_kernel_sizes=[24, 20, 4, 4])),
}


def synth_config(sr: int = 48000, version: str = "v2", spk_embed_dim: int = 109) -> list:
    """The 18-item ``cpt["config"]`` list (``train.py:730``)."""
    t = _SR_TABLE[sr]
    v = t[version]
    return [t["filter_length"] // 2 + 1, 32, 192, 192, 768, 2, 6, 3, 0, "1", [3, 7, 11],
            [[1, 3, 5], [1, 3, 5], [1, 3, 5]], list(v["upsample_rates"]), 512,
            list(v["upsample_kernel_sizes"]), spk_embed_dim, 256, sr]


class _Gen:
    def __init__(self, seed: int):
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def normal(self, shape, std):
        return torch.from_numpy((self.rng.standard_normal(size=shape) * std).astype(np.float32))

    def uniform(self, shape, lo, hi):
        return torch.from_numpy(self.rng.uniform(lo, hi, size=shape).astype(np.float32))


def _wn(g: _Gen, sd, name, shape, std, dim=0):
    """Weight-norm pair: v ~ N(0, std); g = ||v|| * U(0.7, 1.3) (so the fold is exercised)."""
    v = g.normal(shape, std)
    dims = [d for d in range(len(shape)) if d != dim]
    norm = v.pow(2).sum(dim=dims, keepdim=True).sqrt()
    sd[name + ".weight_g"] = norm * g.uniform(norm.shape, 0.7, 1.3)
    sd[name + ".weight_v"] = v


def _conv(g: _Gen, sd, name, co, ci, k, gain=1.0, bias=True):
    sd[name + ".weight"] = g.normal((co, ci, k), gain / math.sqrt(ci * k))
    if bias:
        sd[name + ".bias"] = g.normal((co,), 0.02)


MRF_NAMES = ("MRF-HiFi-GAN", "MRF HiFi-GAN")  # both spellings synthesizers.py:420 accepts
VOCODERS = ("Default",) + MRF_NAMES + ("RefineGAN",)


def _wn_conv(g: _Gen, sd, name, co, ci, k, std, bias=True):
    """A weight-normed Conv1d in the reference's key order (bias, weight_g, weight_v)."""
    if bias:
        sd[name + ".bias"] = g.normal((co,), 0.02)
    _wn(g, sd, name, (co, ci, k), std)


def _dec_nsf(g: _Gen, sd, inter, rks, rds, ur, uic, uks, gin):
    """GeneratorNSF (synthesizers.py:114-161)."""
    sd["dec.m_source.l_linear.weight"] = g.uniform((1, 1), 0.5, 1.5)
    sd["dec.m_source.l_linear.bias"] = g.normal((1,), 0.02)
    _conv(g, sd, "dec.conv_pre", uic, inter, 7)
    nup = len(ur)
    chans = [uic // (2 ** (i + 1)) for i in range(nup)]
    strides = [math.prod(ur[i + 1:]) if i + 1 < nup else 1 for i in range(nup)]
    for i, (u, k) in enumerate(zip(ur, uks)):
        cin = uic // (2 ** i)
        sd[f"dec.ups.{i}.bias"] = g.normal((chans[i],), 0.02)
        _wn(g, sd, f"dec.ups.{i}", (cin, chans[i], k), 1.0 / math.sqrt(cin * k / u))
        s = strides[i]
        kn = 1 if s == 1 else s * 2 - s % 2
        _conv(g, sd, f"dec.noise_convs.{i}", chans[i], 1, kn, gain=0.5)
    j = 0
    for i in range(nup):
        c = chans[i]
        for k, ds in zip(rks, rds):
            for m in range(len(ds)):
                for nm in ("convs1", "convs2"):
                    sd[f"dec.resblocks.{j}.{nm}.{m}.bias"] = g.normal((c,), 0.02)
                    _wn(g, sd, f"dec.resblocks.{j}.{nm}.{m}", (c, c, k), 0.5 / math.sqrt(c * k))
            j += 1
    sd["dec.conv_post.weight"] = g.normal((1, chans[-1], 7), 1.0 / math.sqrt(chans[-1] * 7))
    _conv(g, sd, "dec.cond", uic, gin, 1, gain=0.5)


def _dec_mrf(g: _Gen, sd, inter, rks, rds, ur, uic, uks, gin):
    """HiFiGANMRFGenerator (mrf_hifigan.py:96-120), harmonic_num = 8."""
    sd["dec.m_source.l_linear.weight"] = g.uniform((1, 9), -1.5, 1.5)
    sd["dec.m_source.l_linear.bias"] = g.normal((1,), 0.02)
    _wn_conv(g, sd, "dec.conv_pre", uic, inter, 7, 1.0 / math.sqrt(inter * 7))
    nup = len(ur)
    chans = [uic // (2 ** (i + 1)) for i in range(nup)]
    strides = [math.prod(ur[i + 1:]) if i + 1 < nup else 1 for i in range(nup)]
    for i, (u, k) in enumerate(zip(ur, uks)):
        cin = uic // (2 ** i)
        sd[f"dec.upsamples.{i}.bias"] = g.normal((chans[i],), 0.02)
        _wn(g, sd, f"dec.upsamples.{i}", (cin, chans[i], k), 1.0 / math.sqrt(cin * k / u))
        s = strides[i]
        kn = 1 if s == 1 else s * 2 - s % 2
        _conv(g, sd, f"dec.noise_convs.{i}", chans[i], 1, kn, gain=0.5)
    for i in range(nup):
        c = chans[i]
        for j, (k, ds) in enumerate(zip(rks, rds)):
            for m in range(len(ds)):
                for nm in ("conv1", "conv2"):
                    _wn_conv(g, sd, f"dec.mrfs.{i}.{j}.layers.{m}.{nm}", c, c, k, 0.5 / math.sqrt(c * k))
    _wn_conv(g, sd, "dec.conv_post", 1, chans[-1], 7, 1.0 / math.sqrt(chans[-1] * 7))
    _conv(g, sd, "dec.cond", uic, gin, 1, gain=0.5)


def _dec_refinegan(g: _Gen, sd, inter, ur, gin):
    """RefineGANGenerator (refinegan.py:109-144): 512 initial channels whatever the config says; the config's
    upsample kernel sizes and resblock lists are not read."""
    ch = 512
    sd["dec.m_source.merge.0.weight"] = g.uniform((1, 1), 0.8, 1.6)
    _wn_conv(g, sd, "dec.pre_conv", ch // 2, 1, 7, 2.0 / math.sqrt(7))
    nup = len(ur)
    strides = [math.prod(ur[i + 1:]) if i + 1 < nup else 1 for i in range(nup)]
    for i in range(nup):
        s = strides[i]
        kn = 1 if s == 1 else s * 2 - s % 2
        _wn_conv(g, sd, f"dec.downsample_blocks.{i}", ch // 2 ** (i + 2), 1, kn, 1.0 / math.sqrt(kn))
    _wn_conv(g, sd, "dec.mel_conv", ch // 2, inter, 7, 1.0 / math.sqrt(inter * 7))
    _conv(g, sd, "dec.cond", ch // 2, gin, 1, gain=0.5)
    c = ch
    for i in range(nup):
        new = c // 2
        p = f"dec.upsample_conv_blocks.{i}."
        _conv(g, sd, p + "input_conv", new, c + c // 4, 7)
        for j, k in enumerate((3, 7, 11)):
            # AdaIN weights differ per channel (and per layer): a kernel indexing them wrongly shows
            sd[p + f"blocks.{j}.0.weight"] = g.uniform((new,), 0.05, 0.4)
            for m in range(3):
                for nm in ("convs1", "convs2"):
                    _wn_conv(g, sd, p + f"blocks.{j}.1.{nm}.{m}", new, new, k, 0.5 / math.sqrt(new * k))
            sd[p + f"blocks.{j}.2.weight"] = g.uniform((new,), 0.05, 0.4)
        c = new
    _wn_conv(g, sd, "dec.conv_post", 1, c, 7, 1.0 / math.sqrt(c * 7), bias=False)


def synth_state_dict(cfg: list, seed: int = 1234, emb_dim: int = 768,
                     vocoder: str = "Default") -> "OrderedDict[str, torch.Tensor]":
    """fp32 state dict of ``Synthesizer`` minus ``enc_q`` (``synthesizers.py:396-426``); ``vocoder`` picks the
    decoder's layout as synthesizers.py:418-421 does ("Default" draws exactly what it always drew)."""
    (_, _, inter, hidden, filt, n_heads, n_layers, ksz, _, _, rks, rds, ur, uic, uks, spk, gin, sr) = cfg
    if vocoder not in VOCODERS:
        raise ValueError(f"vocoder must be one of {VOCODERS}, got {vocoder!r}")
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    kc = hidden // n_heads
    # TextEncoder (synthesizers.py:350-371)
    sd["enc_p.emb_phone.weight"] = g.normal((hidden, emb_dim), 1.0 / math.sqrt(emb_dim))
    sd["enc_p.emb_phone.bias"] = g.normal((hidden,), 0.02)
    sd["enc_p.emb_pitch.weight"] = g.normal((256, hidden), 0.1)
    for i in range(n_layers):
        p = f"enc_p.encoder.attn_layers.{i}."
        sd[p + "emb_rel_k"] = g.normal((1, 21, kc), kc ** -0.5)
        sd[p + "emb_rel_v"] = g.normal((1, 21, kc), kc ** -0.5)
        for n in ("q", "k", "v", "o"):
            _conv(g, sd, p + f"conv_{n}", hidden, hidden, 1)
        sd[f"enc_p.encoder.norm_layers_1.{i}.gamma"] = g.uniform((hidden,), 0.8, 1.2)
        sd[f"enc_p.encoder.norm_layers_1.{i}.beta"] = g.normal((hidden,), 0.05)
        _conv(g, sd, f"enc_p.encoder.ffn_layers.{i}.conv_1", filt, hidden, ksz)
        _conv(g, sd, f"enc_p.encoder.ffn_layers.{i}.conv_2", hidden, filt, ksz)
        sd[f"enc_p.encoder.norm_layers_2.{i}.gamma"] = g.uniform((hidden,), 0.8, 1.2)
        sd[f"enc_p.encoder.norm_layers_2.{i}.beta"] = g.normal((hidden,), 0.05)
    _conv(g, sd, "enc_p.proj", inter * 2, hidden, 1, gain=0.5)
    if vocoder in MRF_NAMES:
        _dec_mrf(g, sd, inter, rks, rds, ur, uic, uks, gin)
    elif vocoder == "RefineGAN":
        _dec_refinegan(g, sd, inter, ur, gin)
    else:
        _dec_nsf(g, sd, inter, rks, rds, ur, uic, uks, gin)
    # ResidualCouplingBlock (residuals.py:71-140) + WaveNet (modules.py:9-59)
    half = inter // 2
    for f in range(4):
        p = f"flow.flows.{2 * f}."
        _conv(g, sd, p + "pre", hidden, half, 1)
        for l in range(3):
            sd[p + f"enc.in_layers.{l}.bias"] = g.normal((2 * hidden,), 0.02)
            _wn(g, sd, p + f"enc.in_layers.{l}", (2 * hidden, hidden, 5), 1.0 / math.sqrt(hidden * 5))
            rs = hidden if l == 2 else 2 * hidden
            sd[p + f"enc.res_skip_layers.{l}.bias"] = g.normal((rs,), 0.02)
            _wn(g, sd, p + f"enc.res_skip_layers.{l}", (rs, hidden, 1), 1.0 / math.sqrt(hidden))
        sd[p + "enc.cond_layer.bias"] = g.normal((2 * hidden * 3,), 0.02)
        _wn(g, sd, p + "enc.cond_layer", (2 * hidden * 3, gin, 1), 0.5 / math.sqrt(gin))
        _conv(g, sd, p + "post", half, hidden, 1, gain=0.3)
    sd["emb_g.weight"] = g.normal((spk, gin), 1.0)
    return sd


def make_synth_ckpt(sr: int = 48000, version: str = "v2", seed: int = 1234, vocoder: str = "Default") -> dict:
    """A voice-model checkpoint dict in the ``train.py:729-742`` layout (fp16 weights)."""
    cfg = synth_config(sr, version)
    sd = synth_state_dict(cfg, seed, emb_dim=768 if version == "v2" else 256, vocoder=vocoder)
    opt = OrderedDict(weight=OrderedDict((k, v.half()) for k, v in sd.items()))
    opt["config"] = cfg
    opt["epoch"] = "1epoch"
    opt["step"] = 1
    opt["sr"] = f"{sr // 1000}k"
    opt["f0"] = 1
    opt["version"] = version
    opt["model_name"] = f"synthetic_{sr // 1000}k_{version}_s{seed}"
    opt["vocoder"] = vocoder
    return opt


# ---------------------------------------------------------------- training checkpoints (G_*.pth)
# main/configs/v{1,2}/*.json: "train".segment_size and the "data" section's mel settings, per sample rate
_TRAIN_TABLE = {
    32000: dict(hop_length=320, n_mel_channels=80, segment_size=dict(v1=12800, v2=12800)),
    40000: dict(hop_length=400, n_mel_channels=125, segment_size=dict(v1=12800, v2=12800)),
    48000: dict(hop_length=480, n_mel_channels=128, segment_size=dict(v1=11520, v2=17280)),
}
ENC_Q_LAYERS, ENC_Q_KERNEL = 16, 5  # PosteriorEncoder(spec_channels, inter, hidden, 5, 1, 16) (synthesizers.py:424)


def train_config(sr: int = 40000, version: str = "v2", spk_embed_dim: int = 109) -> dict:
    """The experiment folder's ``config.json`` (main/configs/v{1,2}/{sr}.json) as a dict."""
    t, d = _SR_TABLE[sr], _TRAIN_TABLE[sr]
    v = t[version]
    return {
        "train": {"log_interval": 200, "seed": 1234, "learning_rate": 1e-4, "betas": [0.8, 0.99], "eps": 1e-9,
                  "lr_decay": 0.999875, "segment_size": d["segment_size"][version], "c_mel": 45, "c_kl": 1.0},
        "data": {"max_wav_value": 32768.0, "sample_rate": sr, "filter_length": t["filter_length"],
                 "hop_length": d["hop_length"], "win_length": t["filter_length"],
                 "n_mel_channels": d["n_mel_channels"], "mel_fmin": 0.0, "mel_fmax": None},
        "model": {"inter_channels": 192, "hidden_channels": 192, "filter_channels": 768,
                  "text_enc_hidden_dim": 768 if version == "v2" else 256, "n_heads": 2, "n_layers": 6,
                  "kernel_size": 3, "p_dropout": 0, "resblock": "1", "resblock_kernel_sizes": [3, 7, 11],
                  "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                  "upsample_rates": list(v["upsample_rates"]), "upsample_initial_channel": 512,
                  "upsample_kernel_sizes": list(v["upsample_kernel_sizes"]), "use_spectral_norm": False,
                  "gin_channels": 256, "spk_embed_dim": spk_embed_dim},
    }


def enc_q_state_dict(cfg: list, seed: int = 1234) -> "OrderedDict[str, torch.Tensor]":
    """fp32 state dict of ``Synthesizer.enc_q`` (PosteriorEncoder, synthesizers.py:373-391; WaveNet, modules.py:9-33)
    in the checkpoint's key layout (``.weight_g`` / ``.weight_v``), from a generator of its own: the other
    functions' draws do not move.  The 1x1 ``pre`` conv sees linear magnitudes (peaks of 10^2), so its gain is small
    enough that the gates are not all saturated."""
    spec_channels, inter, hidden, gin = cfg[0], cfg[2], cfg[3], cfg[16]
    g = _Gen(seed ^ 0x51C0DE)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    _conv(g, sd, "enc_q.pre", hidden, spec_channels, 1, gain=0.15)
    for l in range(ENC_Q_LAYERS):
        sd[f"enc_q.enc.in_layers.{l}.bias"] = g.normal((2 * hidden,), 0.02)
        _wn(g, sd, f"enc_q.enc.in_layers.{l}", (2 * hidden, hidden, ENC_Q_KERNEL),
            1.0 / math.sqrt(hidden * ENC_Q_KERNEL))
    for l in range(ENC_Q_LAYERS):
        rs = hidden if l == ENC_Q_LAYERS - 1 else 2 * hidden
        sd[f"enc_q.enc.res_skip_layers.{l}.bias"] = g.normal((rs,), 0.02)
        _wn(g, sd, f"enc_q.enc.res_skip_layers.{l}", (rs, hidden, 1), 0.5 / math.sqrt(hidden))
    sd["enc_q.enc.cond_layer.bias"] = g.normal((2 * hidden * ENC_Q_LAYERS,), 0.02)
    _wn(g, sd, "enc_q.enc.cond_layer", (2 * hidden * ENC_Q_LAYERS, gin, 1), 0.5 / math.sqrt(gin))
    _conv(g, sd, "enc_q.proj", inter * 2, hidden, 1, gain=0.25)
    return sd


def make_train_ckpt(sr: int = 40000, version: str = "v2", seed: int = 1234) -> dict:
    """A generator training checkpoint ``G_*.pth`` as ``save_checkpoint`` writes it (train.py:269-271): fp32
    ``{"model": Synthesizer.state_dict() with .weight_g / .weight_v, "iteration", "optimizer", "learning_rate"}``
    -- ``synth_state_dict`` plus ``enc_q_state_dict``."""
    cfg = synth_config(sr, version)
    sd = synth_state_dict(cfg, seed, emb_dim=768 if version == "v2" else 256)
    sd.update(enc_q_state_dict(cfg, seed))
    return {"model": sd, "iteration": 1, "optimizer": {}, "learning_rate": 1e-4}


def discriminator_state_dict(version: str = "v2", seed: int = 1234) -> "OrderedDict[str, torch.Tensor]":
    """fp32 state dict of ``MultiPeriodDiscriminator(version)`` (train.py:608-674) in the checkpoint's key layout, from
    a generator of its own.  ``weight_v ~ N(0, std)`` with ``std = gain / sqrt(fan_in)``; ``weight_g`` is drawn as
    ``std * sqrt(fan_in) * U(0.7, 1.3)`` -- the expected norm of v times the usual spread, never a computed norm,
    whose f32 summation order differs between hosts: these 71 M parameters regenerate bit for bit from the seed.
    Gains keep the activations O(1) through the six layers: a LeakyReLU(0.1) passes about half the power, so sqrt(2)
    holds a layer's RMS; the first conv of each discriminator sees audio at an RMS of 0.1-0.2 and takes 6."""
    from .discriminator import discriminator_layers
    g = _Gen(seed ^ 0xD15C)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape, _ in discriminator_layers(version):
        fan_in = int(np.prod(shape[1:]))
        gain = 6.0 if name.endswith("convs.0") else 1.0 if name.endswith("conv_post") else math.sqrt(2.0)
        std = gain / math.sqrt(fan_in)
        sd[name + ".bias"] = g.normal((shape[0],), 0.02)
        # std * sqrt(fan_in) is the gain; an elementwise f32 product, the same on every host
        sd[name + ".weight_g"] = g.uniform((shape[0],) + (1,) * (len(shape) - 1), 0.7, 1.3) * float(gain)
        sd[name + ".weight_v"] = g.normal(shape, std)
    return sd


def make_disc_ckpt(version: str = "v2", seed: int = 1234) -> dict:
    """A discriminator training checkpoint ``D_*.pth`` as ``save_checkpoint`` writes it (train.py:269-271)."""
    return {"model": discriminator_state_dict(version, seed), "iteration": 1, "optimizer": {}, "learning_rate": 1e-4}


OPT_STATE_STEP = 1000
OPT_STATE_SCALE = 0.05  # the RMS of the seeded discriminators' gradients on the test signals lies between 5e-3 and 0.3


def discriminator_optimizer_state(version: str = "v2", seed: int = 1234) -> dict:
    """A warm ``torch.optim.AdamW`` state of ``net_d`` after ``OPT_STATE_STEP`` steps, in the layout of
    ``optimizer.state_dict()`` (``{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}``), parameter
    i being the i-th key of ``discriminator_keys(version)`` -- ``net_d.parameters()``' order.  Every value is a NumPy
    draw rounded to f32, so it regenerates bit for bit from the seed: ``exp_avg ~ N(0, 0.05)`` (the scale of the
    gradients) and ``exp_avg_sq = 0.05^2 U(0.25, 4)``."""
    from .discriminator import discriminator_keys
    g = _Gen(seed ^ 0x0ADA)
    state = {}
    keys = discriminator_keys(version)
    for i, shape in enumerate(keys.values()):
        state[i] = {"step": torch.tensor(float(OPT_STATE_STEP)), "exp_avg": g.normal(shape, OPT_STATE_SCALE),
                    "exp_avg_sq": g.uniform(shape, 0.25, 4.0) * float(OPT_STATE_SCALE ** 2)}
    hps = train_config(40000, version)["train"]
    group = {"lr": hps["learning_rate"], "betas": tuple(hps["betas"]), "eps": hps["eps"], "weight_decay": 0.01,
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
             "fused": None, "params": list(range(len(keys)))}
    return {"state": state, "param_groups": [group]}


def write_train_experiment(exp_dir: str, sr: int = 40000, version: str = "v2", frames=(150, 150), seed: int = 1234,
                           sid: int = 3, with_d: bool = False) -> str:
    """A seeded experiment folder as the reference's preprocessing and extraction leave it: ``config.json``,
    ``filelist.txt`` (``wav|phone.npy|pitch.npy|pitchf.npy|sid``), per utterance an IEEE-float wav of
    ``frames[i] * hop`` samples, features of ``frames[i] // 2`` rows (the loader repeats them x2), pitch and pitchf
    of ``frames[i]`` rows with about a quarter unvoiced -- and ``G_1.pth`` (``make_train_ckpt``), whose path is
    returned.  ``with_d`` also writes ``D_1.pth`` (``make_disc_ckpt``) beside it."""
    import json
    import os
    from . import audio_io
    hps = train_config(sr, version)
    hop, emb = hps["data"]["hop_length"], 768 if version == "v2" else 256
    os.makedirs(exp_dir, exist_ok=True)
    with open(os.path.join(exp_dir, "config.json"), "w", encoding="utf-8") as f:
        json.dump(hps, f, indent=1)
    rows = []
    for i, T in enumerate(frames):
        rng = np.random.Generator(np.random.PCG64(seed + 100 + i))
        stem = os.path.join(exp_dir, f"utt{i}")
        audio_io.write_wav_f32(stem + ".wav", synthetic_audio(T * hop / sr + 0.01, seed=seed + i, sr=sr)[:T * hop], sr)
        np.save(stem + "_phone.npy", rng.standard_normal((T // 2, emb)).astype(np.float32))
        np.save(stem + "_pitch.npy", rng.integers(1, 256, size=T).astype(np.int64))
        pitchf = rng.uniform(60, 500, size=T).astype(np.float32)
        pitchf[rng.random(T) < 0.25] = 0.0
        np.save(stem + "_pitchf.npy", pitchf)
        rows.append(f"{stem}.wav|{stem}_phone.npy|{stem}_pitch.npy|{stem}_pitchf.npy|{sid}")
    with open(os.path.join(exp_dir, "filelist.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(rows) + "\n")
    path = os.path.join(exp_dir, "G_1.pth")
    torch.save(make_train_ckpt(sr, version, seed), path)
    if with_d:
        torch.save(make_disc_ckpt(version, seed), os.path.join(exp_dir, "D_1.pth"))
    return path


# ---------------------------------------------------------------- ContentVec
HUBERT_CFG =dict(_name="hubert", label_rate=50, encoder_layers_1=3, logit_temp_ctr=0.1, num_negatives=100,
                  cross_sample_negatives=0, ctr_layers=[-6], extractor_mode="default", encoder_layers=12,
                  encoder_embed_dim=768, encoder_ffn_embed_dim=3072, encoder_attention_heads=12,
                  activation_fn="gelu", layer_type="transformer", dropout=0.1, attention_dropout=0.1,
                  activation_dropout=0.0, encoder_layerdrop=0.0, dropout_input=0.0, dropout_features=0.0,
                  final_dim=256, untie_final_proj=False, layer_norm_first=False,
                  conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", conv_bias=False,
                  conv_pos=128, conv_pos_groups=16, required_seq_len_multiple=2)
FE_LAYERS = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2


def contentvec_state_dict(seed: int = 4321) -> "OrderedDict[str, torch.Tensor]":
    """fp32 ``HubertModel`` state dict (``fairseq.py:1326-1372``), ContentVec shapes."""
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    E, F = 768, 3072
    sd["mask_emb"] = g.uniform((E,), 0, 1)
    sd["label_embs_concat"] = g.uniform((504, 256), 0, 1)
    cin = 1
    for i, (c, k, s) in enumerate(FE_LAYERS):
        sd[f"feature_extractor.conv_layers.{i}.0.weight"] = g.normal((c, cin, k), math.sqrt(2.0 / (cin * k)))
        if i == 0:
            sd["feature_extractor.conv_layers.0.2.weight"] = g.uniform((c,), 0.8, 1.2)
            sd["feature_extractor.conv_layers.0.2.bias"] = g.normal((c,), 0.05)
        cin = c
    sd["layer_norm.weight"] = g.uniform((512,), 0.8, 1.2)
    sd["layer_norm.bias"] = g.normal((512,), 0.05)
    sd["post_extract_proj.weight"] = g.normal((E, 512), 1 / math.sqrt(512))
    sd["post_extract_proj.bias"] = g.normal((E,), 0.02)
    sd["encoder.pos_conv.0.bias"] = g.normal((E,), 0.02)
    _wn(g, sd, "encoder.pos_conv.0", (E, E // 16, 128), math.sqrt(4.0 / (128 * E)), dim=2)
    sd["encoder.layer_norm.weight"] = g.uniform((E,), 0.8, 1.2)
    sd["encoder.layer_norm.bias"] = g.normal((E,), 0.05)
    for i in range(12):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"] = g.normal((E, E), 1 / math.sqrt(E))
            sd[p + f"self_attn.{n}.bias"] = g.normal((E,), 0.02)
        sd[p + "self_attn_layer_norm.weight"] = g.uniform((E,), 0.8, 1.2)
        sd[p + "self_attn_layer_norm.bias"] = g.normal((E,), 0.05)
        sd[p + "fc1.weight"] = g.normal((F, E), 1 / math.sqrt(E))
        sd[p + "fc1.bias"] = g.normal((F,), 0.02)
        sd[p + "fc2.weight"] = g.normal((E, F), 1 / math.sqrt(F))
        sd[p + "fc2.bias"] = g.normal((E,), 0.02)
        sd[p + "final_layer_norm.weight"] = g.uniform((E,), 0.8, 1.2)
        sd[p + "final_layer_norm.bias"] = g.normal((E,), 0.05)
    sd["final_proj.weight"] = g.normal((256, E), 1 / math.sqrt(E))
    sd["final_proj.bias"] = g.normal((256,), 0.02)
    return sd


def make_contentvec_ckpt(seed: int = 4321) -> dict:
    return {"cfg": {"model": dict(HUBERT_CFG), "task": {"sample_rate": 16000}}, "model": contentvec_state_dict(seed)}


# transformers' HubertConfig for the same network (HubertModelWithFinalProj, main/library/utils.py:157-165)
HF_HUBERT_CONFIG = dict(model_type="hubert", architectures=["HubertModelWithFinalProj"], hidden_size=768,
                        num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                        feat_extract_norm="group", feat_extract_activation="gelu", conv_dim=[512] * 7,
                        conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_bias=False,
                        num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, do_stable_layer_norm=False,
                        layer_norm_eps=1e-5, feat_proj_layer_norm=True, classifier_proj_size=256)


def make_hf_hubert(seed: int = 4321) -> tuple[dict, dict]:
    """(config.json dict, state dict) of a transformers-layout ContentVec (``HubertModelWithFinalProj``, the
    ``.safetensors`` embedder of convert.py:342-345) holding the values of ``contentvec_state_dict(seed)`` under
    transformers' parameter names (the weight-norm pair as ``parametrizations.weight.original0 / 1``)."""
    src = contentvec_state_dict(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    sd["masked_spec_embed"] = src["mask_emb"]
    for i in range(len(FE_LAYERS)):
        sd[f"feature_extractor.conv_layers.{i}.conv.weight"] = src[f"feature_extractor.conv_layers.{i}.0.weight"]
    sd["feature_extractor.conv_layers.0.layer_norm.weight"] = src["feature_extractor.conv_layers.0.2.weight"]
    sd["feature_extractor.conv_layers.0.layer_norm.bias"] = src["feature_extractor.conv_layers.0.2.bias"]
    sd["feature_projection.layer_norm.weight"] = src["layer_norm.weight"]
    sd["feature_projection.layer_norm.bias"] = src["layer_norm.bias"]
    sd["feature_projection.projection.weight"] = src["post_extract_proj.weight"]
    sd["feature_projection.projection.bias"] = src["post_extract_proj.bias"]
    sd["encoder.pos_conv_embed.conv.bias"] = src["encoder.pos_conv.0.bias"]
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = src["encoder.pos_conv.0.weight_g"]
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = src["encoder.pos_conv.0.weight_v"]
    sd["encoder.layer_norm.weight"] = src["encoder.layer_norm.weight"]
    sd["encoder.layer_norm.bias"] = src["encoder.layer_norm.bias"]
    for i in range(12):
        a, b = f"encoder.layers.{i}.", f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            for t in ("weight", "bias"):
                sd[f"{b}attention.{n}.{t}"] = src[f"{a}self_attn.{n}.{t}"]
        for hf, fs in (("layer_norm", "self_attn_layer_norm"), ("feed_forward.intermediate_dense", "fc1"),
                       ("feed_forward.output_dense", "fc2"), ("final_layer_norm", "final_layer_norm")):
            for t in ("weight", "bias"):
                sd[f"{b}{hf}.{t}"] = src[f"{a}{fs}.{t}"]
    sd["final_proj.weight"] = src["final_proj.weight"]
    sd["final_proj.bias"] = src["final_proj.bias"]
    return dict(HF_HUBERT_CONFIG), sd


# ---------------------------------------------------------------- RMVPE
def _bn(g: _Gen, sd, name, c):
    sd[name + ".weight"] = g.uniform((c,), 0.8, 1.2)
    sd[name + ".bias"] = g.normal((c,), 0.05)
    sd[name + ".running_mean"] = g.normal((c,), 0.05)
    sd[name + ".running_var"] = g.uniform((c,), 0.5, 1.5)
    sd[name + ".num_batches_tracked"] = torch.tensor(100, dtype=torch.long)


def _conv2(g: _Gen, sd, name, co, ci, k, bias=False, gain=1.0):
    sd[name + ".weight"] = g.normal((co, ci, k, k), gain * math.sqrt(2.0 / (ci * k * k)))
    if bias:
        sd[name + ".bias"] = g.normal((co,), 0.02)


def _cbr(g: _Gen, sd, name, ci, co):
    """ConvBlockRes (RMVPE.py:11-22)."""
    _conv2(g, sd, name + ".conv.0", co, ci, 3, gain=0.7)
    _bn(g, sd, name + ".conv.1", co)
    _conv2(g, sd, name + ".conv.3", co, co, 3, gain=0.7)
    _bn(g, sd, name + ".conv.4", co)
    if ci != co:
        _conv2(g, sd, name + ".shortcut", co, ci, 1, bias=True, gain=0.7)


def rmvpe_state_dict(seed: int = 777) -> "OrderedDict[str, torch.Tensor]":
    """fp32 ``E2E(4, 1, (2, 2))`` state dict (``RMVPE.py:125-144,254-260``)."""
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    nb = 4
    _bn(g, sd, "unet.encoder.bn", 1)
    ci, co = 1, 16
    for l in range(5):
        for b in range(nb):
            _cbr(g, sd, f"unet.encoder.layers.{l}.conv.{b}", ci if b == 0 else co, co)
        ci, co = co, co * 2
    ci, co = 256, 512
    for l in range(4):
        for b in range(nb):
            _cbr(g, sd, f"unet.intermediate.layers.{l}.conv.{b}", (ci if l == 0 else co) if b == 0 else co, co)
    cin = 512
    for l in range(5):
        cout = cin // 2
        sd[f"unet.decoder.layers.{l}.conv1.0.weight"] = g.normal((cin, cout, 3, 3), math.sqrt(2.0 / (cin * 9 / 4)) * 0.7)
        _bn(g, sd, f"unet.decoder.layers.{l}.conv1.1", cout)
        for b in range(nb):
            _cbr(g, sd, f"unet.decoder.layers.{l}.conv2.{b}", cout * 2 if b == 0 else cout, cout)
        cin = cout
    _conv2(g, sd, "cnn", 3, 16, 3, bias=True)
    H, I = 256, 384
    for sfx in ("", "_reverse"):
        sd[f"fc.0.gru.weight_ih_l0{sfx}"] = g.normal((3 * H, I), 1 / math.sqrt(I))
        sd[f"fc.0.gru.weight_hh_l0{sfx}"] = g.normal((3 * H, H), 1 / math.sqrt(H))
        sd[f"fc.0.gru.bias_ih_l0{sfx}"] = g.normal((3 * H,), 0.05)
        sd[f"fc.0.gru.bias_hh_l0{sfx}"] = g.normal((3 * H,), 0.05)
    sd["fc.1.weight"] = g.normal((360, 512), 1 / math.sqrt(512))
    sd["fc.1.bias"] = g.normal((360,), 0.05)
    return sd


# ---------------------------------------------------------------- CREPE
CREPE_CAPACITY = {
    "full": ([1, 1024, 128, 128, 128, 256], [1024, 128, 128, 128, 256, 512], 2048),
    "large": ([1, 768, 96, 96, 96, 192], [768, 96, 96, 96, 192, 384], 1536),
    "medium": ([1, 512, 64, 64, 64, 128], [512, 64, 64, 64, 128, 256], 1024),
    "small": ([1, 256, 32, 32, 32, 64], [256, 32, 32, 32, 64, 128], 512),
    "tiny": ([1, 128, 16, 16, 16, 32], [128, 16, 16, 16, 32, 64], 256),
}


def crepe_state_dict(seed: int = 999, capacity: str = "full") -> "OrderedDict[str, torch.Tensor]":
    """fp32 ``Crepe(capacity)`` state dict (``CREPE.py:11-58``): conv{i} (k x 1 kernels), conv{i}_BN,
    classifier."""
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    cin, cout, nfeat = CREPE_CAPACITY[capacity]
    for i in range(6):
        k = 512 if i == 0 else 64
        sd[f"conv{i + 1}.weight"] = g.normal((cout[i], cin[i], k, 1), math.sqrt(2.0 / (cin[i] * k)))
        sd[f"conv{i + 1}.bias"] = g.normal((cout[i],), 0.02)
        _bn(g, sd, f"conv{i + 1}_BN", cout[i])
    sd["classifier.weight"] = g.normal((360, nfeat), 2.0 / math.sqrt(nfeat))
    sd["classifier.bias"] = g.normal((360,), 0.5)
    return sd


FCPE_MEL = {"type": "default", "sr": 16000, "num_mels": 128, "n_fft": 1024, "win_size": 1024, "hop_size": 160,
            "fmin": 0, "fmax": 8000}
# gains of the synthetic FCPE: default-scale weights decode every frame to one bin, so the body convs are scaled
# up until the argmax moves with the input, and the output bias puts the confidence threshold (0.006) inside
# the range the top latent covers (tests/golden/make_golden_fcpe.py asserts what the fixture needs)
FCPE_BODY_GAIN, FCPE_OUT_GAIN, FCPE_OUT_BIAS = 1.0, 3.0, -14.6


def fcpe_checkpoint(seed: int = 2028, n_layers: int = 6, hidden_dims: int = 512,
                    use_harmonic_emb: bool = False) -> dict:
    """A seeded ``fcpe.pt`` in the reference's layout (FCPE.py:807-810): {"config_dict": {"mel", "model"},
    "model": CFNaiveMelPE.state_dict()} of a conv-only model (tests/golden/fcpe_keys.json lists the keys)."""
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    C, f0_min, f0_max = hidden_dims, 32.70, 1975.5
    cents = [1200 * torch.log2(torch.Tensor([f]) / 10)[0] for f in (f0_min, f0_max)]
    sd["cent_table"] = torch.linspace(cents[0], cents[1], 360)
    sd["gaussian_blurred_cent_mask"] = (1200 * torch.log2(torch.Tensor([f0_max / 10.])))[0]
    if use_harmonic_emb:
        sd["harmonic_emb.weight"] = g.normal((9, C), 0.1)

    def norm(name):
        sd[name + ".weight"] = g.uniform((C,), 0.7, 1.3)
        sd[name + ".bias"] = g.normal((C,), 0.1)

    # the log-mel input is mostly a constant floor (log 1e-5 in the empty bands): taps that sum to zero pass on
    # only what changes from frame to frame, or the constant part would decide every frame's argmax alike
    _conv(g, sd, "input_stack.0", C, 128, 3)
    sd["input_stack.0.weight"] -= sd["input_stack.0.weight"].mean(dim=2, keepdim=True)
    norm("input_stack.1")
    _conv(g, sd, "input_stack.3", C, C, 3, gain=FCPE_BODY_GAIN)
    for i in range(n_layers):
        p = f"net.encoder_layers.{i}."
        norm(p + "conformer.net.0")
        _conv(g, sd, p + "conformer.net.2", 4 * C, C, 1, gain=FCPE_BODY_GAIN)
        _conv(g, sd, p + "conformer.net.4.conv", 2 * C, 1, 31, gain=FCPE_BODY_GAIN)
        _conv(g, sd, p + "conformer.net.6", C, 2 * C, 1, gain=FCPE_BODY_GAIN)
        norm(p + "norm")  # the attention branch's LayerNorm: unused when conv_only
    norm("norm")
    sd["output_proj.bias"] = g.normal((360,), 0.5) + FCPE_OUT_BIAS
    v = g.normal((360, C), 1.0 / math.sqrt(C))
    sd["output_proj.parametrizations.weight.original0"] = \
        v.pow(2).sum(dim=1, keepdim=True).sqrt() * g.uniform((360, 1), 0.7, 1.3) * FCPE_OUT_GAIN
    sd["output_proj.parametrizations.weight.original1"] = v
    model = {"type": "CFNaiveMelPE", "out_dims": 360, "hidden_dims": C, "n_layers": n_layers, "n_heads": 8,
             "f0_min": f0_min, "f0_max": f0_max, "use_fa_norm": False, "conv_only": True, "conv_dropout": 0.1,
             "atten_dropout": 0.1, "use_harmonic_emb": bool(use_harmonic_emb)}
    return {"config_dict": {"mel": dict(FCPE_MEL), "model": model}, "model": sd}


# gains of the synthetic FCPE_LEGACY (tests/golden/make_golden_fcpe_legacy.py asserts what the fixtures need): the
# first conv's zero-mean taps are scaled so that the frames differ, dense_out so that the argmax moves, and the
# output bias puts the legacy threshold (0.03) inside the range the top latent covers
FCPE_LEGACY_IN_GAIN, FCPE_LEGACY_BODY_GAIN, FCPE_LEGACY_OUT_GAIN, FCPE_LEGACY_OUT_BIAS = 3.0, 0.15, 3.0, -12.8
FCPE_LEGACY_FEATURES = 266  # int(64 * ln 64), FastAttention's default


def fcpe_legacy_checkpoint(seed: int = 3031, n_layers: int = 6, n_chans: int = 512,
                           nb_features: int = FCPE_LEGACY_FEATURES, out_bias: float = FCPE_LEGACY_OUT_BIAS) -> dict:
    """A seeded ``fcpe_legacy.pt`` in the reference's layout (FCPE.py:778-782): {"config": {"model", "loss"},
    "model": FCPE_LEGACY.state_dict()} (tests/golden/fcpe_legacy_keys.json lists the keys).  The Performer
    projections [nb_features][64] (Gaussian rows made orthogonal in blocks of 64, as FastAttention draws them) are
    weights: drawn once from the seed."""
    g = _Gen(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    C, f0_min, f0_max, inner = n_chans, 32.70, 1975.5, 512
    cents = [1200 * torch.log2(torch.Tensor([f]) / 10)[0] for f in (f0_min, f0_max)]
    sd["cent_table"] = torch.from_numpy(np.linspace(float(cents[0]), float(cents[1]), 360).astype(np.float32))

    def norm(name):
        sd[name + ".weight"] = g.uniform((C,), 0.7, 1.3)
        sd[name + ".bias"] = g.normal((C,), 0.1)

    def linear(name, co, ci, gain=1.0):
        sd[name + ".weight"] = g.normal((co, ci), gain / math.sqrt(ci))
        sd[name + ".bias"] = g.normal((co,), 0.02)

    def projection():
        blocks = []
        for r0 in range(0, nb_features, 64):
            qm, _ = np.linalg.qr(g.rng.standard_normal((64, 64)))
            blocks.append(qm.T[:min(64, nb_features - r0)])
        scale = np.linalg.norm(g.rng.standard_normal((nb_features, 64)), axis=1)
        return torch.from_numpy((scale[:, None] * np.concatenate(blocks)).astype(np.float32))

    _conv(g, sd, "stack.0", C, 128, 3, gain=FCPE_LEGACY_IN_GAIN)
    sd["stack.0.weight"] -= sd["stack.0.weight"].mean(dim=2, keepdim=True)  # see fcpe_checkpoint
    norm("stack.1")
    _conv(g, sd, "stack.3", C, C, 3)
    for i in range(n_layers):
        p = f"decoder._layers.{i}."
        norm(p + "conformer.net.0")
        _conv(g, sd, p + "conformer.net.2", 4 * C, C, 1)
        _conv(g, sd, p + "conformer.net.4.conv", 2 * C, 1, 31)
        _conv(g, sd, p + "conformer.net.6", C, 2 * C, 1, gain=FCPE_LEGACY_BODY_GAIN)
        norm(p + "norm")
        sd[p + "attn.fast_attention.projection_matrix"] = projection()
        linear(p + "attn.to_q", inner, C)
        linear(p + "attn.to_k", inner, C)
        linear(p + "attn.to_v", inner, C)
        linear(p + "attn.to_out", C, inner, gain=FCPE_LEGACY_BODY_GAIN)
    norm("norm")
    sd["dense_out.bias"] = g.normal((360,), 0.5) + out_bias
    v = g.normal((360, C), 1.0 / math.sqrt(C))
    sd["dense_out.parametrizations.weight.original0"] = \
        v.pow(2).sum(dim=1, keepdim=True).sqrt() * g.uniform((360, 1), 0.7, 1.3) * FCPE_LEGACY_OUT_GAIN
    sd["dense_out.parametrizations.weight.original1"] = v
    model = {"input_channel": 128, "out_dims": 360, "n_layers": n_layers, "n_chans": C, "use_siren": False,
             "use_full": False, "confidence": False, "threshold": 0.05, "use_input_conv": True}
    loss = {"loss_mse_scale": 10, "loss_l2_regularization": False, "loss_l2_regularization_scale": 1,
            "loss_grad1_mse": False, "loss_grad1_mse_scale": 1}
    return {"config": {"model": model, "loss": loss}, "model": sd}


# ---------------------------------------------------------------- audio
def synthetic_audio(seconds: float, seed: int = 1000, sr: int = 16000) -> np.ndarray:
    """SURVEY §8(d) test signal: 3-harmonic glide (60-240 Hz) + 200 ms gaps every 5 s + noise, peak <= 0.9."""
    n = int(round(seconds * sr))
    t = np.arange(n, dtype=np.float64) / sr
    f0 = 120.0 * 2.0 ** np.sin(2 * np.pi * 0.25 * t)
    phi = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(0.5 ** (h - 1) * np.sin(h * phi) for h in (1, 2, 3)) * 0.3
    env = np.ones(n)
    for s0 in np.arange(5.0, seconds, 5.0):
        a, b = int((s0 - 0.1) * sr), int((s0 + 0.1) * sr)
        env[max(a, 0):min(b, n)] = 0.0
    rng = np.random.Generator(np.random.PCG64(seed))
    x = env * x + 0.003 * rng.standard_normal(n)
    peak = np.abs(x).max()
    if peak > 0.9:
        x *= 0.9 / peak
    return x.astype(np.float32)


def silence_layout_audio(layout, seed: int = 5000, sr: int = 16000, floor: float = 1e-5) -> np.ndarray:
    """Test signal for the silence slicer (edges.py): ``layout`` = [(seconds, voiced?), ...]; voiced
    spans are the §8(d) glide, silent spans seeded noise at ``floor`` (≈ -100 dBFS, no exact ties)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = []
    for k, (sec, voiced) in enumerate(layout):
        n = int(round(sec * sr))
        if voiced:
            parts.append(synthetic_audio(sec, seed=seed + 1 + k, sr=sr)[:n].astype(np.float64))
        else:
            parts.append(floor * rng.standard_normal(n))
    return np.concatenate(parts).astype(np.float32)


# slicer cases: leading / short (< max_sil_kept) / medium (1-2x) / long (> 2x) middle silences, trailing
SLICER_LAYOUTS = {
    "mixed": [(1.0, 0), (6.0, 1), (0.7, 0), (6.0, 1), (7.0, 0), (6.0, 1), (11.0, 0), (5.0, 1), (2.0, 0)],
    "no_silence": [(8.0, 1)],
    "short_input": [(0.5, 0), (3.0, 1)],
    "lead_long": [(12.0, 0), (6.0, 1), (0.3, 0), (2.0, 1)],
}
