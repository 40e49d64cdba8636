"""The training step's forward and its losses on the MI355X (main/inference/train.py).

What runs here is ``net_g(...)`` of ``train.py:843`` -- ``Synthesizer.forward`` (synthesizers.py:434-442): the prior
encoder, the posterior encoder ``enc_q`` and its sample, the random segment slice, the NSF decoder on the slice, the
flow in the forward direction -- plus the linear and mel spectrograms (``train.py:700-716``) and ``loss_mel`` /
``loss_kl`` as the training loop logs them (``train.py:844-848, 865-866``).  With a ``D_*.pth`` beside the ``G_*.pth``
(``rvc_amd.discriminator``), also ``net_d`` on the wave slice and ``y_hat`` and the GAN losses ``loss_disc``,
``loss_gen``, ``loss_fm`` and ``loss_gen_all`` (``train.py:850-869``): the number the reference keeps its
``lowest_value`` on and the two series its overtraining detector smooths.  On top of that:

* ``evaluate``         scores a ``G_*.pth``, or a (G, D) pair, on an experiment folder's filelist (which checkpoint is
                       best, is it overtraining) --
                       ``python -m rvc_amd.train_forward --exp DIR --ckpt G_123.pth [--d-ckpt D_123.pth]``;
* ``write_spec_cache`` writes the ``*.spec.pt`` files the reference's loader otherwise computes on the CPU in its
                       first epoch (``train.py:377-393``).

One utterance per call (B = 1, no padding): every mask of the reference is all ones, and its padded batch computes
the same values on an utterance's valid frames.  No generator backward pass or optimizer step, no AMP;
without ``d_step`` both of the loop's ``net_d`` passes see the saved D, with it D takes its own step
between them; the MRF-HiFi-GAN and RefineGAN decoders are refused here.  The kernels are csrc/trainfwd.hip and csrc/discriminator.hip; the encoder, flow, decoder and most of the
discriminators' layers run on the conv engine as ``SynthesizerAMD`` does.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import melbasis, ops
from .synth import SynthesizerAMD, fold_weight_norm

ENC_Q_LAYERS = 16  # PosteriorEncoder(spec_channels, inter, hidden, 5, 1, 16) (synthesizers.py:424)
OFF_SLICE = 1 << 38  # Philox counter offset of the slice-start draw under an utterance's seed (z: 0, sine: 1 << 40)
MAX_FRAMES = 900  # get_labels' cap (train.py:374)


def enc_q_keys(n_layers: int = ENC_Q_LAYERS) -> list:
    """The checkpoint keys of ``enc_q`` this loader reads (``save_checkpoint``'s layout, train.py:269-271)."""
    keys = ["enc_q.pre.weight", "enc_q.pre.bias"]
    for name in ("in_layers", "res_skip_layers"):
        for l in range(n_layers):
            keys += [f"enc_q.enc.{name}.{l}.bias", f"enc_q.enc.{name}.{l}.weight_g", f"enc_q.enc.{name}.{l}.weight_v"]
    keys += ["enc_q.enc.cond_layer.bias", "enc_q.enc.cond_layer.weight_g", "enc_q.enc.cond_layer.weight_v",
             "enc_q.proj.weight", "enc_q.proj.bias"]
    return keys


def config_list(hps: dict) -> list:
    """The ``Synthesizer(*args)`` list train.py builds from config.json (:730, with the training segment in frames)."""
    d, m, t = hps["data"], hps["model"], hps["train"]
    return [d["filter_length"] // 2 + 1, t["segment_size"] // d["hop_length"], m["inter_channels"],
            m["hidden_channels"], m["filter_channels"], m["n_heads"], m["n_layers"], m["kernel_size"], m["p_dropout"],
            m["resblock"], m["resblock_kernel_sizes"], m["resblock_dilation_sizes"], m["upsample_rates"],
            m["upsample_initial_channel"], m["upsample_kernel_sizes"], m["spk_embed_dim"], m["gin_channels"],
            d["sample_rate"]]


def slice_start(u: torch.Tensor, T: int, S: int) -> torch.Tensor:
    """rand_slice_segments' start (commons.py:31): the f32 product ``u * (T - S + 1)`` truncated to int64."""
    return (u.to(torch.float32) * (T - S + 1)).to(torch.int64)


def check_supported(model: dict, hps: dict, vocoder: str = "Default", f0: bool = True) -> None:
    """What the training forward refuses, by name, before anything is uploaded."""
    if float(hps["model"]["p_dropout"]) != 0.0:
        raise NotImplementedError(f"rvc_amd: p_dropout = {hps['model']['p_dropout']}: the training forward runs the "
                                  "model in train mode, where a non-zero dropout is random; only p_dropout = 0 "
                                  "(every shipped config) is on the device")
    if not f0 or "enc_p.emb_pitch.weight" not in model:
        raise NotImplementedError("rvc_amd: no-f0 models (the reference's Generator without pitch guidance) are not "
                                  "in the training forward")
    if vocoder != "Default":
        raise NotImplementedError(f"rvc_amd: vocoder {vocoder!r}: only the Default (NSF-HiFiGAN) decoder is in the "
                                  "training forward; MRF-HiFi-GAN and RefineGAN are not")
    missing = [k for k in enc_q_keys() if k not in model]
    if missing:
        raise KeyError(f"rvc_amd: not a training checkpoint: enc_q keys missing ({missing[:3]} ...)")


class TrainSynthAMD(SynthesizerAMD):
    """``Synthesizer`` in ``.train()`` mode at p_dropout 0, forward only, from a training checkpoint
    ``{"model": state_dict, ...}`` (train.py:269-271) and the experiment's config.json dict."""

    def __init__(self, ckpt: dict, hps: dict, device: str = "cuda", vocoder: str = "Default", f0: bool = True):
        model = ckpt["model"]
        check_supported(model, hps, vocoder, f0)
        cfg = config_list(hps)
        emb = model["enc_p.emb_phone.weight"].shape[1]
        super().__init__({"weight": {k: v for k, v in model.items() if not k.startswith("enc_q.")}, "config": cfg,
                          "f0": 1, "version": "v2" if emb == 768 else "v1", "vocoder": "Default"}, device)
        self.hps = hps
        self.spec_channels, self.segment_frames = cfg[0], cfg[1]
        self.hop = hps["data"]["hop_length"]
        if self.upp != self.hop:
            raise ValueError(f"rvc_amd: the decoder upsamples by {self.upp}, the spectrogram hops {self.hop}")
        W = fold_weight_norm({k: model[k] for k in enc_q_keys()})
        H, dev = self.hidden, device
        Conv = ops.Conv
        self.q_pre = Conv(W["enc_q.pre.weight"], W["enc_q.pre.bias"], device=dev)
        self.q_ins, self.q_rs_a, self.q_rs_b = [], [], []
        for l in range(ENC_Q_LAYERS):
            p = "enc_q.enc."
            self.q_ins.append(Conv(W[p + f"in_layers.{l}.weight"], W[p + f"in_layers.{l}.bias"], device=dev))
            rw, rb = W[p + f"res_skip_layers.{l}.weight"], W[p + f"res_skip_layers.{l}.bias"]
            if l < ENC_Q_LAYERS - 1:
                self.q_rs_a.append(Conv(rw[:H], rb[:H], device=dev))
                self.q_rs_b.append(Conv(rw[H:], rb[H:], device=dev))
            else:
                self.q_rs_b.append(Conv(rw, rb, device=dev))
        self.q_cond = Conv(W["enc_q.enc.cond_layer.weight"], W["enc_q.enc.cond_layer.bias"], device=dev)
        self.q_proj = Conv(W["enc_q.proj.weight"], W["enc_q.proj.bias"], device=dev)

    # ------------------------------------------------------------------ stages
    def speaker(self, sid: int):
        """g = emb_g(sid) [gin][1] (synthesizers.py:435)."""
        return self.emb_g[int(sid)].view(self.gin, 1)

    def _wavenet(self, h, ins, rs_a, rs_b, g_all, T):
        """WaveNet.forward (modules.py:35-51) in place on h [H][T] at an all-ones mask; g_all = cond_layer(g), layer
        l's slice entering its in_layer as a second bias -> the skip sum [1][H][T]."""
        H, dev, n = self.hidden, h.device, len(ins)
        acts = torch.empty(1, H, T, device=dev)
        out_acc = torch.empty(1, H, T, device=dev)
        for l in range(n):
            xin = ins[l](h, pad=(ins[l].K - 1) // 2, bias2=g_all[l * 2 * H:(l + 1) * 2 * H])
            ops.gate(xin, acts, 1, H, T)
            if l < n - 1:
                rs_a[l](acts, out=h, res=h)
            rs_b[l](acts, out=out_acc, accumulate=(l > 0))
        return out_acc

    def posterior(self, spec, g, noise):
        """PosteriorEncoder.forward (synthesizers.py:387-391): spec [K][T], g [gin][1], noise [inter][T] (the
        reference's randn_like draw) -> z, m_q, logs_q, each [1][inter][T]."""
        K, T = spec.shape[-2], spec.shape[-1]
        if K != self.spec_channels:
            raise ValueError(f"posterior: spec has {K} bins, the model expects {self.spec_channels}")
        I, H, dev = self.inter, self.hidden, spec.device
        h = torch.empty(1, H, T, device=dev)
        self.q_pre(spec.reshape(1, K, T).contiguous(), out=h)
        skip = self._wavenet(h, self.q_ins, self.q_rs_a, self.q_rs_b, self.q_cond(g).view(-1), T)
        stats = self.q_proj(skip).view(1, 2 * I, T)
        z = torch.empty(1, I, T, device=dev)
        ops.prior_sample(stats, noise.reshape(1, I, T).contiguous(), z, 1, I, T, 1.0)  # m + noise * exp(logs)
        return z, stats[:, :I], stats[:, I:]

    def _flow_forward(self, z, gc, T):
        """ResidualCouplingBlock.forward (residuals.py:87-90, 127-136, mean_only): per layer x1 += post(WN(pre(x0))),
        then the flip; z [1][inter][T] is left as it is."""
        H, I, half, dev = self.hidden, self.inter, self.inter // 2, z.device
        bufs = (z.clone(), torch.empty(1, I, T, device=dev))
        h = torch.empty(1, H, T, device=dev)
        x = bufs[0]
        for f in range(4):
            F = self.flows[f]
            F["pre"](x, B=1, Lin=T, x_bstride=I * T, out=h)  # x0 = x[:, :half]
            skip = self._wavenet(h, F["ins"], F["rs_a"], F["rs_b"], gc[f * 6 * H:(f + 1) * 6 * H], T)
            x1 = x[:, half:]
            F["post"](skip, out=x1, res=x1, y_bstride=I * T, res_bstride=I * T, out_scale=1.0)
            nxt = bufs[1] if x is bufs[0] else bufs[0]
            ops.flip_channels(x, nxt, 1, I, T)
            x = nxt
        return x

    def flow_forward(self, z, g):
        """z [1][inter][T], g [gin][1] -> z_p [1][inter][T]."""
        T = z.shape[-1]
        return self._flow_forward(z.reshape(1, self.inter, T).contiguous(), self.cond(g).view(-1), T)

    # ------------------------------------------------------------------ Synthesizer.forward
    def forward(self, phone, pitch, pitchf, spec, sid, ids_slice=None, z_noise=None, sine_noise=None,
                sine_phase=None, seed: int = 0):
        """``Synthesizer.forward`` (synthesizers.py:434-442) on one utterance: phone [T][E], pitch int64 [T], pitchf
        f32 [T], spec [K][T] (device tensors; a leading batch axis of 1 is accepted), sid an int ->
        ``(y_hat [S * hop], ids_slice int64 [1], (z, z_p, m_p, logs_p, m_q, logs_q))``, the six each [1][inter][T].

        Parity inputs, otherwise drawn on the device from ``seed`` (Philox, as ``infer`` does): ``z_noise``
        [inter][T] the posterior's randn_like, ``ids_slice`` the slice start (else ``floor(u * (T - S + 1))`` of one
        uniform draw, commons.py:31), ``sine_noise`` [S * hop] the source's randn_like.  ``sine_phase`` is accepted
        and unused: the NSF source zeroes its only harmonic's initial phase (synthesizers.py:87-88)."""
        I, S = self.inter, self.segment_frames
        T = spec.shape[-1]
        dev = spec.device
        if T < S:
            raise ValueError(f"forward: {T} frames are fewer than the training segment's {S}")
        E = phone.shape[-1]
        if E != self.emb_dim or phone.numel() != T * E or pitch.numel() != T or pitchf.numel() != T:
            raise ValueError("forward: phone [T][E], pitch [T], pitchf [T] must match the spectrogram's T frames")
        sid = int(sid.reshape(-1)[0]) if torch.is_tensor(sid) else int(sid)
        g = self.speaker(sid)
        gc = self.cond(g).view(-1)
        phone_cf = torch.empty(E, T, device=dev)
        ops.transpose(phone.reshape(T, E).contiguous().float(), phone_cf, 1, T, E)
        stats_p = self.text_encoder(phone_cf.view(1, E, T), pitch.reshape(T).to(torch.int64).contiguous(), T)
        if z_noise is None:
            z_noise = ops.randn(torch.empty(1, I, T, device=dev), seed, 0)
        z, m_q, logs_q = self.posterior(spec, g, z_noise.to(dev, torch.float32))
        z_p = self._flow_forward(z, gc, T)
        if ids_slice is None:
            u = ops.rand_uniform(torch.empty(1, device=dev), seed, OFF_SLICE)
            ids_slice = slice_start(u, T, S)
        else:
            ids_slice = torch.as_tensor(ids_slice, dtype=torch.int64).reshape(1).to(dev)
        st = int(ids_slice.item())
        if not 0 <= st <= T - S:
            raise ValueError(f"forward: slice start {st} outside [0, {T - S}]")
        L = S * self.upp
        if sine_noise is None:
            sine_noise = ops.randn(torch.empty(1, L, device=dev), seed, ops.OFF_SINE)
        elif sine_noise.numel() != L:
            raise ValueError(f"forward: sine_noise has {sine_noise.numel()} values, the slice {L} samples")
        z_slice = z[:, :, st:st + S].contiguous()
        f0_slice = pitchf.reshape(T)[st:st + S].float().contiguous().view(1, S)
        y_hat = self.generator(z_slice, f0_slice, gc[4 * 6 * self.hidden:], S,
                               sine_noise.to(dev, torch.float32).reshape(1, L).contiguous(), 1)
        return y_hat.view(L), ids_slice, (z, z_p, stats_p[:, :I], stats_p[:, I:], m_q, logs_q)


# ---------------------------------------------------------------------- spectrograms (train.py:700-716)
_BASIS = {}


def mel_basis(sr, n_fft, n_mels, fmin, fmax, device):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) at its defaults (Slaney scale and norm) on the device,
    uploaded once per setting; ``fmax=None`` is sr / 2.  ``melbasis`` restates librosa."""
    key = (sr, n_fft, n_mels, float(fmin), None if fmax is None else float(fmax), str(device))
    if key not in _BASIS:
        b = melbasis.mel_filterbank(sr, n_fft, n_mels, float(fmin), sr / 2.0 if fmax is None else float(fmax),
                                    htk=False)
        _BASIS[key] = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(device)
    return _BASIS[key]


def spectrogram(y, n_fft, hop_size, win_size=None):
    """``spectrogram_torch`` (train.py:700-706, center=False): y [B][N] f32 on the device -> [B][n_fft/2+1][F]."""
    if win_size is not None and win_size != n_fft:
        raise NotImplementedError(f"rvc_amd: spectrogram with win_size {win_size} != n_fft {n_fft} (no shipped "
                                  "config has one)")
    return ops.spectrogram(y.float().contiguous(), n_fft, hop_size)


def spec_to_mel(spec, n_fft, num_mels, sample_rate, fmin, fmax):
    """``spec_to_mel_torch`` (train.py:708-713): spec [B][K][F] -> log(max(basis @ spec, 1e-5)) [B][M][F]."""
    s3 = spec if spec.dim() == 3 else spec.unsqueeze(0)
    return ops.mel_log(s3.contiguous(), mel_basis(sample_rate, n_fft, num_mels, fmin, fmax, spec.device))


def mel_spectrogram(y, n_fft, num_mels, sample_rate, hop_size, win_size, fmin, fmax):
    """``mel_spectrogram_torch`` (train.py:715-716)."""
    return spec_to_mel(spectrogram(y, n_fft, hop_size, win_size), n_fft, num_mels, sample_rate, fmin, fmax)


def _losses(hps, spec, y_hat, ids_slice, z_p, logs_q, m_p, logs_p):
    """(l1, kl) device scalars from a forward's outputs (train.py:844-848, 865-866 before c_mel / c_kl)."""
    d = hps["data"]
    args = (d["filter_length"], d["n_mel_channels"], d["sample_rate"], d["mel_fmin"], d["mel_fmax"])
    mel = spec_to_mel(spec, *args)
    y_hat_mel = mel_spectrogram(y_hat.view(1, -1), args[0], args[1], args[2], d["hop_length"], d["win_length"],
                                args[3], args[4])
    return ops.slice_l1(mel, ids_slice, y_hat_mel), ops.kl_loss(z_p, logs_q, m_p, logs_p)


def generator_losses(model: TrainSynthAMD, phone, pitch, pitchf, spec, sid, cfg: dict = None, **draws) -> dict:
    """``loss_mel`` and ``loss_kl`` of one utterance as the training loop computes them (train.py:843-848, 865-866):
    ``{"loss_mel": c_mel * l1_loss(y_mel, y_hat_mel), "loss_kl": c_kl * kl_loss(...)}`` (f32 products, as floats).
    ``cfg`` is the config.json dict (default: the model's); ``draws`` go to ``TrainSynthAMD.forward``."""
    hps = cfg or model.hps
    y_hat, ids, (z, z_p, m_p, logs_p, m_q, logs_q) = model.forward(phone, pitch, pitchf, spec, sid, **draws)
    l1, kl = _losses(hps, spec, y_hat, ids, z_p, logs_q, m_p, logs_p)
    both = torch.cat([l1, kl]).cpu().numpy()
    return {"loss_mel": float(both[0] * np.float32(hps["train"]["c_mel"])),
            "loss_kl": float(both[1] * np.float32(hps["train"]["c_kl"]))}


D_LOSSES = ("loss_disc", "loss_gen", "loss_fm")  # the new per-utterance scalars, each aggregated as a plain mean


def step_losses(model: TrainSynthAMD, disc, phone, pitch, pitchf, spec, wave, sid, cfg: dict = None, d_step: bool = False,
                d_snapshot: dict = None, **draws) -> dict:
    """Every loss of one training step on one utterance (train.py:843-869): the forward, ``wave`` [T * hop] sliced at
    ``ids_slice * hop`` for ``segment_size`` samples (train.py:850), ``disc`` (a ``DiscriminatorAMD``) on that slice
    and ``y_hat`` -> ``DiscriminatorAMD.losses``' dict with ``loss_mel``, ``loss_kl`` and ``loss_gen_all`` (floats, one
    host read).  ``loss_mel`` and ``loss_kl`` are the bits ``generator_losses`` returns for the same draws.

    ``d_step`` (``disc`` a ``DiscriminatorTrainerAMD``): D takes its optimizer step on this pair between the two passes,
    as the loop does (train.py:851-863) -- ``loss_disc`` and its lists are the first pass', ``loss_gen``, ``loss_fm`` and
    ``loss_gen_all`` see the stepped D, ``grad_norm_d`` is added -- and D is put back (to ``d_snapshot``, or to what it
    was on entry), so the numbers do not depend on what was scored before."""
    hps = cfg or model.hps
    y_hat, ids, (z, z_p, m_p, logs_p, m_q, logs_q) = model.forward(phone, pitch, pitchf, spec, sid, **draws)
    l1, kl = _losses(hps, spec, y_hat, ids, z_p, logs_q, m_p, logs_p)
    seg, st = y_hat.numel(), int(ids.item()) * model.hop
    wave = wave.reshape(-1)
    if st + seg > wave.numel():
        raise ValueError(f"step_losses: the wave has {wave.numel()} samples, the slice ends at {st + seg}")
    wave = wave[st:st + seg].float().contiguous()
    c_mel, c_kl = float(hps["train"]["c_mel"]), float(hps["train"]["c_kl"])
    if not d_step:
        return disc.losses(wave, y_hat, l1, kl, c_mel, c_kl)
    snap = d_snapshot if d_snapshot is not None else disc.snapshot()
    try:
        first = disc.step([(wave, y_hat)])
        out = disc.losses(wave, y_hat, l1, kl, c_mel, c_kl)
    finally:
        disc.restore(snap)
    out.update(first)
    return out


def aggregate_gan(per_utt: list) -> dict:
    """The new losses over utterances: each the plain mean (every slice has ``segment_size`` samples, so a batch's
    means are the means of the utterances' means), and ``loss_gen_all`` the sum of the four aggregates (train.py:869).
    per_utt: ``aggregate``'s dicts with ``loss_disc``, ``loss_gen`` and ``loss_fm`` added."""
    if not per_utt:
        return {k: None for k in D_LOSSES + ("loss_gen_all",)}
    out = {k: sum(u[k] for u in per_utt) / len(per_utt) for k in D_LOSSES}
    base = aggregate(per_utt)
    out["loss_gen_all"] = out["loss_gen"] + out["loss_fm"] + base["loss_mel"] + base["loss_kl"]
    return out


# ---------------------------------------------------------------------- experiment folders
def read_filelist(path: str) -> list:
    """filelist.txt rows ``wav|phone.npy|pitch.npy|pitchf.npy|sid`` (train.py:282-284, 342)."""
    rows = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f):
            line = line.strip()
            if not line:
                continue
            parts = line.split("|")
            if len(parts) != 5:
                raise ValueError(f"{path}:{n + 1}: expected wav|phone|pitch|pitchf|sid, got {len(parts)} fields")
            rows.append(tuple(parts))
    return rows


def parse_sid(sid: str) -> int:
    """get_sid (train.py:350-356): a speaker id that is no integer reads as 0."""
    try:
        return int(sid)
    except ValueError:
        return 0


def trim_labels(phone: np.ndarray, pitch: np.ndarray, pitchf: np.ndarray, spec_frames: int):
    """get_labels and the length trim of get_audio_text_pair (train.py:358-375): phone frames repeated x2, all three
    capped at 900 frames, then everything cut to the shorter of phone and spectrogram -> (phone, pitch, pitchf, T)."""
    phone = np.repeat(phone, 2, axis=0)
    n = min(phone.shape[0], MAX_FRAMES)
    phone, pitch, pitchf = phone[:n], pitch[:n], pitchf[:n]
    T = min(phone.shape[0], spec_frames)
    return phone[:T], pitch[:T], pitchf[:T], T


def aggregate(per_utt: list) -> dict:
    """What one reference batch of these utterances would log: ``l1_loss`` over equal-sized slices is the mean of the
    utterances' means, ``kl_loss`` the summed KL over the summed mask, ``sum(kl_i * T_i) / sum(T_i)``.  per_utt:
    dicts with ``loss_mel``, ``loss_kl`` (already times c_mel / c_kl) and ``frames``."""
    if not per_utt:
        return {"loss_mel": None, "loss_kl": None}
    frames = sum(u["frames"] for u in per_utt)
    return {"loss_mel": sum(u["loss_mel"] for u in per_utt) / len(per_utt),
            "loss_kl": sum(u["loss_kl"] * u["frames"] for u in per_utt) / frames}


def _load_hps(exp_dir):
    with open(os.path.join(exp_dir, "config.json"), encoding="utf-8") as f:
        return json.load(f)


def _spec_of(wav_path, hps, device):
    from . import audio_io
    d = hps["data"]
    x, sr = audio_io.read_wav(wav_path)
    if sr != d["sample_rate"]:
        raise ValueError(f"{wav_path}: sample rate {sr}, the experiment's is {d['sample_rate']}")
    if x.ndim != 1:
        raise ValueError(f"{wav_path}: expected a mono wav")
    return spectrogram(torch.from_numpy(np.ascontiguousarray(x)).to(device).view(1, -1), d["filter_length"],
                       d["hop_length"], d["win_length"])[0]


def write_spec_cache(exp_dir: str, device: str = "cuda") -> dict:
    """For each wav of ``exp_dir/filelist.txt`` write ``<wav>.spec.pt`` next to it as train.py:381, 391-392 does: the
    CPU f32 spectrogram [n_fft/2+1][F] through ``torch.save(..., _use_new_zipfile_serialization=False)``.  Files
    that exist are left alone.  -> {"written": n, "skipped": n}."""
    hps = _load_hps(exp_dir)
    written = skipped = 0
    seen = set()
    for wav, *_ in read_filelist(os.path.join(exp_dir, "filelist.txt")):
        path = wav.replace(".wav", ".spec.pt")
        if path in seen:
            continue
        seen.add(path)
        if os.path.exists(path):
            skipped += 1
            continue
        torch.save(_spec_of(wav, hps, device).cpu(), path, _use_new_zipfile_serialization=False)
        written += 1
    return {"written": written, "skipped": skipped}


def _wave_of(wav_path, device):
    from . import audio_io
    x, _ = audio_io.read_wav(wav_path)
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)


def evaluate(exp_dir: str, checkpoint, limit: int = None, seed: int = 0, device: str = "cuda",
             vocoder: str = "Default", d_checkpoint=None, d_step: bool = False) -> dict:
    """Score a generator checkpoint (a ``G_*.pth`` path, its loaded dict, or a built ``TrainSynthAMD``) on the
    utterances of ``exp_dir/filelist.txt``: per-utterance ``loss_mel`` / ``loss_kl`` and the aggregates one reference
    batch of them would log (``aggregate``).  Utterance i of the filelist draws from ``seed + i``, so its numbers do
    not depend on ``limit`` or on the others; utterances shorter than the training segment are skipped and counted.

    ``d_checkpoint`` (a ``D_*.pth`` path, its loaded dict, or a built ``DiscriminatorAMD``): the entries and the
    aggregates also carry ``loss_disc``, ``loss_gen``, ``loss_fm`` and ``loss_gen_all`` (``step_losses``,
    ``aggregate_gan``), the entries the per-discriminator lists too.  Without it the result is what it always was.

    ``d_step`` (needs ``d_checkpoint``: a path, a dict or a built ``DiscriminatorTrainerAMD``): per utterance D takes
    its optimizer step on that utterance's pair before ``loss_gen`` / ``loss_fm`` / ``loss_gen_all`` are taken, as the
    training loop logs them (``step_losses``), the entries carry ``grad_norm_d``, and D is restored after each."""
    if d_step and d_checkpoint is None:
        raise ValueError("rvc_amd: d_step needs d_checkpoint (the D_*.pth whose step is taken)")
    hps = _load_hps(exp_dir)
    if d_step and hps["train"].get("fp16_run"):
        raise NotImplementedError("rvc_amd: fp16_run / AMP training: the discriminator's step on the device is f32")
    if isinstance(checkpoint, TrainSynthAMD):
        model = checkpoint
    else:
        ck = torch.load(checkpoint, map_location="cpu", weights_only=False) if isinstance(checkpoint, str) \
            else checkpoint
        model = TrainSynthAMD(ck, hps, device, vocoder=vocoder)
    disc = None
    if d_checkpoint is not None:
        from .discriminator import DiscriminatorAMD, DiscriminatorTrainerAMD
        disc = d_checkpoint
        if not isinstance(disc, DiscriminatorAMD):
            dk = torch.load(disc, map_location="cpu", weights_only=False) if isinstance(disc, str) else disc
            disc = DiscriminatorTrainerAMD(dk, model.version, hps["train"], device) if d_step else \
                DiscriminatorAMD(dk, model.version, device)
        elif d_step and not isinstance(disc, DiscriminatorTrainerAMD):
            raise TypeError("rvc_amd: d_step needs a DiscriminatorTrainerAMD (a DiscriminatorAMD holds no optimizer)")
    snap = disc.snapshot() if d_step else None
    rows = read_filelist(os.path.join(exp_dir, "filelist.txt"))
    if limit is not None:
        rows = rows[:limit]
    S = model.segment_frames
    per_utt, skipped = [], 0
    for i, (wav, phone_p, pitch_p, pitchf_p, sid) in enumerate(rows):
        spec = _spec_of(wav, hps, device)
        phone, pitch, pitchf, T = trim_labels(np.load(phone_p), np.load(pitch_p), np.load(pitchf_p), spec.shape[-1])
        if T < S:
            skipped += 1
            continue
        args = (torch.from_numpy(phone.astype(np.float32)).to(device),
                torch.from_numpy(pitch.astype(np.int64)).to(device),
                torch.from_numpy(pitchf.astype(np.float32)).to(device), spec[:, :T].contiguous())
        if disc is None:
            losses = generator_losses(model, *args, parse_sid(sid), hps, seed=seed + i)
        else:
            extra = {"d_step": True, "d_snapshot": snap} if d_step else {}
            losses = step_losses(model, disc, *args, _wave_of(wav, device), parse_sid(sid), hps, seed=seed + i, **extra)
        per_utt.append({"index": i, "wav": wav, "frames": T, **losses})
    out = aggregate(per_utt)
    if disc is not None:
        out.update(aggregate_gan(per_utt))
    if d_step:
        out["grad_norm_d"] = sum(u["grad_norm_d"] for u in per_utt) / len(per_utt) if per_utt else None
    out.update(utterances=per_utt, scored=len(per_utt), skipped=skipped)
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="loss_mel / loss_kl of generator checkpoints on an experiment folder; "
                                             "with their D_*.pth also loss_disc / loss_gen / loss_fm / loss_gen_all")
    ap.add_argument("--exp", required=True, help="experiment folder (config.json, filelist.txt)")
    ap.add_argument("--ckpt", required=True, action="append", help="G_*.pth (repeatable)")
    ap.add_argument("--d-ckpt", action="append", default=None,
                    help="D_*.pth, once per --ckpt and paired with them in order")
    ap.add_argument("--d-step", action="store_true",
                    help="step D on each utterance's pair before loss_gen / loss_fm, as the training loop logs them; "
                         "adds grad_norm_d (needs --d-ckpt)")
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.d_ckpt is not None and len(a.d_ckpt) != len(a.ckpt):
        ap.error(f"--d-ckpt was given {len(a.d_ckpt)} times, --ckpt {len(a.ckpt)}: one D per G, in order")
    if a.d_step and a.d_ckpt is None:
        ap.error("--d-step requires --d-ckpt")
    for n, ck in enumerate(a.ckpt):
        dk = a.d_ckpt[n] if a.d_ckpt is not None else None
        extra = {"d_step": True} if a.d_step else {}
        r = evaluate(a.exp, ck, a.limit, a.seed, a.device, d_checkpoint=dk, **extra)
        line = {"checkpoint": ck, "loss_mel": r["loss_mel"], "loss_kl": r["loss_kl"],
                "scored": r["scored"], "skipped": r["skipped"]}
        if dk is not None:
            line.update(d_checkpoint=dk, **{k: r[k] for k in D_LOSSES + ("loss_gen_all",)})
        if a.d_step:
            line.update(grad_norm_d=r["grad_norm_d"])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
