"""Golden vectors of the training forward: the REFERENCE itself, in f32 and in f64 with the f32 run's draws replayed.

Run in the survey container only (it needs the reference tree ``make_golden.py`` points at):

    python tests/golden/make_golden_train_forward.py

What runs is ``Synthesizer.forward`` in ``.train()`` mode (synthesizers.py:434-442) and ``main/inference/train.py``'s
own ``spectrogram_torch``, ``spec_to_mel_torch``, ``mel_spectrogram_torch``, ``slice_segments`` and ``kl_loss``, in the
order of the training loop (train.py:843-848, 865-866), on the seeded weights of ``rvc_amd.synthetic.make_train_ckpt``
loaded the way ``load_checkpoint`` loads a ``G_*.pth`` (train.py:257-263).  ``train.py`` parses its arguments and opens
``assets/logs/<name>/config.json`` when imported, so the harness sets ``sys.argv``, writes that file, and stubs
``torch.utils.tensorboard``; ``librosa.filters.mel`` is ``rvc_amd.melbasis`` (Slaney scale, ``fmax=None`` read as
sr / 2), so parity against librosa itself stays unpinned, as for RMVPE.

Per case two files (one would pass the repository's 1 MiB limit for a committed file):

* ``train_forward_<case>.npz``: the inputs (wav, phone, pitch, pitchf, sid), the four draws in draw order,
  ``ids_slice``, the f64 run's ``m_q``, ``logs_q``, ``z``, ``z_p``, ``y_hat``, ``y_mel``, ``y_hat_mel``, both runs'
  ``loss_mel`` / ``loss_kl``, ``ref_dev``: per stage the f32 run's RMS and max deviation from the f64 run, with
  the f64 stage's RMS and max magnitude; and every ``.weight_g`` of the checkpoint (``wg_*``): ``synthetic`` takes
  them from an f32 torch reduction whose order follows the host's vector width, so a host may regenerate them one
  bit off, and the tests put the recorded ones back (``train_forward_ref.fixture_ckpt``);
* ``train_forward_<case>_spec.npz``: the f64 run's linear spectrogram.

The f32 run's tensors are not stored: the tests measure against the f64 stages, and ``ref_dev`` holds what the f32 run
is good for.  ``enc_q_keys.json``: the keys and shapes of the reference ``enc_q``'s own ``state_dict()`` in the
checkpoint's naming.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from rvc_amd import melbasis, synthetic  # noqa: E402

OUT = mg.OUT
STAGES = ("spec", "m_q", "logs_q", "z", "z_p", "y_hat", "y_mel", "y_hat_mel")
#        name  sr     version  T   seed
CASES = [("a", 40000, "v2", 48, 4101),
         ("b", 48000, "v2", 45, 4102),   # odd T, slice start > 0
         ("c", 32000, "v1", 40, 4103)]   # T == S: the start must be 0


def stub_for_train():
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb

    def mel(sr, n_fft, n_mels, fmin=0.0, fmax=None, htk=False, **kw):
        return melbasis.mel_filterbank(sr, n_fft, n_mels, fmin, sr / 2.0 if fmax is None else fmax, htk=htk)

    sys.modules["librosa.filters"].mel = mel


def import_train(work, hps):
    exp = os.path.join(work, "assets", "logs", "golden")
    os.makedirs(exp, exist_ok=True)
    with open(os.path.join(exp, "config.json"), "w") as f:
        json.dump(hps, f)
    sys.argv = ["train.py", "--model_name", "golden", "--save_every_epoch", "1", "--sample_rate",
                str(hps["data"]["sample_rate"])]
    return importlib.import_module("main.inference.train")


class Replay:
    """torch.randn_like / torch.rand hand back the recorded draws, in the dtype asked of them."""

    def __init__(self, draws, dtype):
        self.draws, self.dtype, self.i = draws, dtype, 0
        self._rl, self._r = torch.randn_like, torch.rand

    def _next(self, kind):
        k, v = self.draws[self.i]
        assert k == kind, (k, kind)
        self.i += 1
        return v.to(self.dtype)

    def __enter__(self):
        def rl(x, *a, **k):
            out = self._next("randn_like")
            assert out.shape == x.shape
            return out

        torch.randn_like = rl
        torch.rand = lambda *a, **k: self._next("rand")
        return self

    def __exit__(self, *a):
        torch.randn_like, torch.rand = self._rl, self._r


def step(train, net_g, hps, wav, phone, pitch, pitchf, sid):
    """train.py:843-848, 865-866 on one utterance -> the stages and the two losses."""
    from torch.nn import functional as F
    d, t = hps["data"], hps["train"]
    S = t["segment_size"] // d["hop_length"]
    spec = train.spectrogram_torch(wav, d["filter_length"], d["hop_length"], d["win_length"], center=False)
    T = spec.shape[-1]
    lens = torch.tensor([T])
    y_hat, ids_slice, _, z_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net_g(phone, lens, pitch, pitchf, spec, lens, sid)
    mel_args = (d["filter_length"], d["n_mel_channels"], d["sample_rate"], d["mel_fmin"], d["mel_fmax"])
    mel = train.spec_to_mel_torch(spec, *mel_args)
    y_mel = train.slice_segments(mel, ids_slice, S, dim=3)
    y_hat_mel = train.mel_spectrogram_torch(y_hat.squeeze(1), mel_args[0], mel_args[1], mel_args[2], d["hop_length"],
                                            d["win_length"], mel_args[3], mel_args[4])
    loss_mel = F.l1_loss(y_mel, y_hat_mel) * t["c_mel"]
    loss_kl = train.kl_loss(z_p, logs_q, m_p, logs_p, z_mask) * t["c_kl"]
    assert bool(z_mask.all())
    return dict(spec=spec, m_q=m_q, logs_q=logs_q, z=z, z_p=z_p, y_hat=y_hat, y_mel=y_mel, y_hat_mel=y_hat_mel,
                m_p=m_p, logs_p=logs_p, loss_mel=loss_mel, loss_kl=loss_kl, ids_slice=ids_slice)


def build_ref_net(train, hps, ck, emb):
    """The reference Synthesizer in .train() mode, a G_*.pth dict loaded as load_checkpoint does (train.py:257-263)."""
    from main.library.algorithm.synthesizers import Synthesizer
    from rvc_amd.train_forward import config_list
    net_g = Synthesizer(*config_list(hps), use_f0=True, text_enc_hidden_dim=emb, vocoder="Default",
                        checkpointing=False)
    sd = train.replace_keys_in_dict(train.replace_keys_in_dict(dict(ck["model"]), ".weight_v",
                                                               ".parametrizations.weight.original1"),
                                    ".weight_g", ".parametrizations.weight.original0")
    missing, unexpected = net_g.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return net_g.train().float()


def gen_case(train, work, name, sr, version, T, seed):
    hps = synthetic.train_config(sr, version)
    d = hps["data"]
    hop, S = d["hop_length"], hps["train"]["segment_size"] // d["hop_length"]
    train.mel_basis.clear()  # keyed by fmax, dtype and device only: one run of the reference has one config
    train.hann_window.clear()
    emb = 768 if version == "v2" else 256
    ck = synthetic.make_train_ckpt(sr, version, seed)
    net_g = build_ref_net(train, hps, ck, emb)
    wg = {k: v.numpy().reshape(-1) for k, v in ck["model"].items() if k.endswith(".weight_g")}

    rng = np.random.Generator(np.random.PCG64(seed + 1))
    wav = synthetic.synthetic_audio(T * hop / sr + 0.01, seed=seed, sr=sr)[:T * hop][None]
    phone = rng.standard_normal((1, T, emb)).astype(np.float32)
    pitch = rng.integers(1, 256, size=(1, T)).astype(np.int64)
    pitchf = rng.uniform(60, 500, size=(1, T)).astype(np.float32)
    pitchf[:, rng.random(T) < 0.25] = 0.0  # unvoiced frames, as gen_synth
    sid = np.array([3], dtype=np.int64)
    args = [torch.from_numpy(a) for a in (wav, phone, pitch, pitchf, sid)]

    torch.manual_seed(seed + 2)
    with torch.no_grad(), mg.NoiseRecorder() as rec:
        r32 = step(train, net_g, hps, *args)
    kinds = [(k, tuple(v.shape)) for k, v in rec.draws]
    assert kinds == [("randn_like", (1, 192, T)), ("rand", (1,)), ("rand", (1, 1, 1)),
                     ("randn_like", (1, S * hop, 1))], kinds
    assert r32["spec"].shape[-1] == T
    net64 = net_g.double()
    a64 = [a.double() if a.dtype == torch.float32 else a for a in args]
    with torch.no_grad(), Replay(rec.draws, torch.float64) as rp:
        r64 = step(train, net64, hps, *a64)
    assert rp.i == 4
    assert torch.equal(r32["ids_slice"], r64["ids_slice"])
    start = int(r32["ids_slice"][0])
    assert 0 <= start <= T - S and (start > 0 if name == "b" else True) and (start == 0 if T == S else True), start

    ref_dev = {}
    for k in STAGES:
        a, b = r32[k].double(), r64[k]
        e = a - b
        ref_dev[k] = [float(e.pow(2).mean().sqrt()), float(e.abs().max()), float(b.pow(2).mean().sqrt()),
                      float(b.abs().max())]
    np.savez_compressed(
        os.path.join(OUT, f"train_forward_{name}.npz"), sr=sr, version=version, seed=seed, T=T, S=S,
        wav=wav, phone=phone, pitch=pitch, pitchf=pitchf, sid=sid,
        z_noise=rec.draws[0][1].numpy(), slice_u=rec.draws[1][1].numpy(), sine_phase=rec.draws[2][1].numpy(),
        sine_noise=rec.draws[3][1].numpy(), ids_slice=r32["ids_slice"].numpy(),
        **{k + "_f64": r64[k].numpy() for k in STAGES if k != "spec"},
        loss_mel_f32=np.float32(r32["loss_mel"]), loss_kl_f32=np.float32(r32["loss_kl"]),
        loss_mel_f64=np.float64(r64["loss_mel"]), loss_kl_f64=np.float64(r64["loss_kl"]),
        wg_keys=np.array(list(wg)), wg_sizes=np.array([v.size for v in wg.values()]),
        wg_values=np.concatenate(list(wg.values())), ref_dev_stages=np.array(STAGES), ref_dev=np.array([ref_dev[k] for k in STAGES]))
    np.savez_compressed(os.path.join(OUT, f"train_forward_{name}_spec.npz"), spec_f64=r64["spec"].numpy())
    print(name, "start", start, "loss_mel", float(r32["loss_mel"]), float(r64["loss_mel"]), "loss_kl",
          float(r32["loss_kl"]), float(r64["loss_kl"]))
    for k in STAGES:
        print("   %-10s rms dev %.3e max dev %.3e | rms %.3e max %.3e" % (k, *ref_dev[k]))
    return net_g


def main():
    work = mg.setup_harness()
    stub_for_train()
    train = import_train(work, synthetic.train_config(40000, "v2"))
    for case in CASES:
        net_g = gen_case(train, work, *case)
    # enc_q's key table, from the last reference module itself, in the checkpoint's naming (train.py:271)
    sd = train.replace_keys_in_dict(train.replace_keys_in_dict(
        {k: v for k, v in net_g.state_dict().items() if k.startswith("enc_q.")},
        ".parametrizations.weight.original1", ".weight_v"), ".parametrizations.weight.original0", ".weight_g")
    with open(os.path.join(OUT, "enc_q_keys.json"), "w") as f:
        json.dump({"32000/v1": {k: list(v.shape) for k, v in sd.items()}}, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
