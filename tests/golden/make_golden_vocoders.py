"""Golden vectors for the MRF-HiFi-GAN and RefineGAN decoders, from the REFERENCE's own Synthesizer on CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_vocoders.py

``Synthesizer(..., vocoder=...).infer`` on the seeded synthetic checkpoints (``synthetic.make_synth_ckpt(vocoder=)``),
as ``make_golden.gen_synth`` does for the default decoder.  The large draws are not stored: during the run
``torch.randn_like`` / ``torch.rand`` return ``draw(draw_seed, index, kind, shape)`` below, and the tests regenerate
them with the same rule.  Each ``.npz`` holds the inputs, ``har`` (the source module's output), ``z``, ``z_p``,
``m_p``, ``logs_p``, ``o`` and ``har_ref_spread``: the RMS between the source module run in float32 and a float64
copy of it on the same inputs and draws -- the reference's own precision, which bounds what ``har`` can be held to.
``vocoder_keys.json`` is the key -> shape table of the reference modules' own ``state_dict()`` (``enc_q`` dropped,
weight-norm keys renamed as train.py:742 saves them).
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np
import torch

import make_golden as mg
from make_golden import OUT, synthetic


_RAND, _RANDN = torch.rand, torch.randn  # the real ones (SeededDraws patches torch.rand)


def draw(draw_seed: int, index: int, kind: str, shape) -> torch.Tensor:
    """The index-th draw of a run: f32 from a torch.Generator seeded by (draw_seed, index)."""
    g = torch.Generator().manual_seed(draw_seed * 1000 + index)
    fn = _RAND if kind == "rand" else _RANDN
    return fn(*shape, generator=g, dtype=torch.float32)


class SeededDraws:
    """Replaces torch.randn_like / torch.rand with ``draw`` keyed by draw index (``start`` = the first index)."""

    def __init__(self, draw_seed, start=0):
        self.seed, self.n, self.log = draw_seed, start, []
        self._rl, self._r = torch.randn_like, torch.rand

    def __enter__(self):
        def rl(t, *a, **k):
            out = draw(self.seed, self.n, "randn", tuple(t.shape)).to(t.dtype)
            self.log.append(("randn_like", tuple(t.shape)))
            self.n += 1
            return out

        def r(*shape, dtype=None, **k):
            out = draw(self.seed, self.n, "rand", tuple(shape))
            self.log.append(("rand", tuple(shape)))
            self.n += 1
            return out.to(dtype) if dtype is not None else out

        torch.randn_like, torch.rand = rl, r
        return self

    def __exit__(self, *a):
        torch.randn_like, torch.rand = self._rl, self._r


def build_ref(ckpt):
    from main.library.algorithm.synthesizers import Synthesizer
    version = ckpt["version"]
    net_g = Synthesizer(*ckpt["config"], use_f0=1, text_enc_hidden_dim=768 if version == "v2" else 256,
                        vocoder=ckpt["vocoder"], checkpointing=False)
    del net_g.enc_q
    missing, unexpected = net_g.load_state_dict(ckpt["weight"], strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return net_g.eval().float()


def key_table(sr, version, vocoder):
    """key -> shape of the reference module's own state_dict() in the saved checkpoint's naming."""
    from main.library.algorithm.synthesizers import Synthesizer
    cfg = synthetic.synth_config(sr, version)
    net_g = Synthesizer(*cfg, use_f0=1, text_enc_hidden_dim=768 if version == "v2" else 256, vocoder=vocoder,
                        checkpointing=False)
    del net_g.enc_q
    out = {}
    for k, v in net_g.state_dict().items():
        k = k.replace(".parametrizations.weight.original1", ".weight_v")
        k = k.replace(".parametrizations.weight.original0", ".weight_g")
        out[k] = list(v.shape)
    return out


def rms(a, b=None):
    a = a.detach().double()
    if b is not None:
        a = a - b.detach().double()
    return float(a.pow(2).mean().sqrt())


def gen(name, vocoder, sr, version, T, seed):
    ckpt = synthetic.make_synth_ckpt(sr, version, seed=seed, vocoder=vocoder)
    net_g = build_ref(ckpt)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    emb = 768 if version == "v2" else 256
    phone = rng.standard_normal((1, T, emb)).astype(np.float32)
    pitch = rng.integers(1, 256, size=(1, T)).astype(np.int64)
    pitchf = rng.uniform(60, 500, size=(1, T)).astype(np.float32)
    pitchf[:, rng.random(T) < 0.25] = 0.0  # unvoiced frames
    sid = np.array([3], dtype=np.int64)
    draw_seed = seed + 2
    seen = {}
    src = net_g.dec.m_source
    h1 = src.register_forward_pre_hook(lambda m, a: seen.__setitem__("src_in", a[0].detach().clone()))
    h2 = src.register_forward_hook(lambda m, a, out: seen.__setitem__("har", out.detach().clone()))
    with torch.no_grad(), SeededDraws(draw_seed) as rec:
        o, x_mask, (z, z_p, m_p, logs_p) = net_g.infer(torch.from_numpy(phone), torch.tensor([T]),
                                                       torch.from_numpy(pitch), torch.from_numpy(pitchf),
                                                       torch.from_numpy(sid))
    h1.remove()
    h2.remove()
    kinds = [k for k, _ in rec.log]
    n_adain = 6 * len(ckpt["config"][12]) if vocoder == "RefineGAN" else 0
    assert kinds == ["randn_like", "rand", "randn_like"] + ["randn_like"] * n_adain, kinds
    # the source module in float64 on the same inputs and draws (draws 1 and 2)
    src64 = copy.deepcopy(src).double()
    with torch.no_grad(), SeededDraws(draw_seed, start=1):
        har64 = src64(seen["src_in"].double())
    har = seen["har"]
    spread = rms(har, har64)
    o_rms, o_max = rms(o), float(o.abs().max())
    print(f"{name}: o rms {o_rms:.4f} max {o_max:.4f}  har rms {rms(har):.4f}  har_ref_spread {spread:.3e}  "
          f"draws {len(kinds)}")
    assert o_rms > 0.01 and o_max < 0.999, "the reference's output is silent or saturated: adjust the synthetic scales"
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), sr=sr, version=version, seed=seed, T=T, vocoder=vocoder,
                        draw_seed=draw_seed, n_draws=len(kinds), phone=phone, pitch=pitch, pitchf=pitchf, sid=sid,
                        har=har.reshape(1, -1).numpy(), har_ref_spread=spread, o=o.numpy(), z=z.numpy(),
                        z_p=z_p.numpy(), m_p=m_p.numpy(), logs_p=logs_p.numpy())


def main():
    mg.setup_harness()
    gen("mrf_48k_v2", "MRF-HiFi-GAN", 48000, "v2", 37, 31)
    gen("mrf_40k_v2", "MRF HiFi-GAN", 40000, "v2", 24, 32)
    gen("refinegan_48k_v2", "RefineGAN", 48000, "v2", 37, 33)
    gen("refinegan_32k_v2", "RefineGAN", 32000, "v2", 24, 34)
    tables = {}
    for vocoder in ("MRF-HiFi-GAN", "RefineGAN"):
        for sr, version in ((48000, "v2"), (32000, "v1")):
            tables[f"{vocoder}/{sr}/{version}"] = key_table(sr, version, vocoder)
    with open(os.path.join(OUT, "vocoder_keys.json"), "w") as f:
        json.dump(tables, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
