"""Host-side checks of the MRF-HiFi-GAN / RefineGAN support: synthetic checkpoint layouts against the reference
modules' own key tables, the Default layout unchanged, the goldens' source output against the float64 restatement
the GPU op test uses, and the model-level C API's refusal."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import vocoder_util as vu
from rvc_amd import synthetic
from rvc_amd.synth import fold_weight_norm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# sha256 over (key, dtype, shape, bytes) of make_synth_ckpt(...)["weight"] in key order, computed on the commit before
# the vocoder argument existed
PARENT_HASH = {(48000, "v2", 1234): "1d439f908b56ecf30917153f7bfbbeac77dcda46bf7eccbb4ba98fc6d4376a66",
               (32000, "v1", 7): "efe5219b5b331a92b20894b6dcc444d771191457f3949e8fa6647b34534dbc6f"}


def ckpt_hash(ck):
    h = hashlib.sha256()
    for k, v in ck["weight"].items():
        h.update(k.encode())
        h.update(str(v.dtype).encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("key", list(PARENT_HASH))
def test_default_checkpoint_is_unchanged(key):
    sr, version, seed = key
    ck = synthetic.make_synth_ckpt(sr, version, seed)
    assert ck["vocoder"] == "Default"
    assert ckpt_hash(ck) == PARENT_HASH[key]
    assert ckpt_hash(synthetic.make_synth_ckpt(sr, version, seed, vocoder="Default")) == PARENT_HASH[key]


@pytest.mark.parametrize("vocoder", ["MRF-HiFi-GAN", "MRF HiFi-GAN", "RefineGAN"])
@pytest.mark.parametrize("sr,version", [(48000, "v2"), (32000, "v1")])
def test_synthetic_checkpoint_has_the_reference_layout(vocoder, sr, version):
    """Exactly the key set and shapes of the reference module's own state_dict() (tests/golden/vocoder_keys.json,
    written by make_golden_vocoders.py)."""
    tables = json.load(open(os.path.join(GOLDEN, "vocoder_keys.json")))
    want = tables[f"{'MRF-HiFi-GAN' if vocoder.startswith('MRF') else vocoder}/{sr}/{version}"]
    ck = synthetic.make_synth_ckpt(sr, version, seed=3, vocoder=vocoder)
    assert ck["vocoder"] == vocoder
    got = {k: list(v.shape) for k, v in ck["weight"].items()}
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert got == want
    assert all(v.dtype == torch.float16 for v in ck["weight"].values())


def test_refinegan_adain_weights_differ_per_channel():
    W = synthetic.make_synth_ckpt(48000, "v2", seed=3, vocoder="RefineGAN")["weight"]
    ws = [v for k, v in W.items() if ".blocks." in k and k.endswith((".0.weight", ".2.weight"))]
    assert len(ws) == 4 * 3 * 2
    for w in ws:
        assert w.float().unique().numel() > w.numel() // 2


def test_unknown_vocoder_is_refused():
    with pytest.raises(ValueError):
        synthetic.make_synth_ckpt(48000, "v2", seed=3, vocoder="BigVGAN")


@pytest.mark.parametrize("name", vu.GOLDENS)
def test_harmonic_source_restatement_matches_reference_golden(golden, name):
    """The float64 numpy restatement of the source module (vocoder_util.np_harmonic_source, the GPU op test's
    reference) against the reference's own ``har``: within 4 x the reference's float32-vs-float64 spread (floor 1e-6),
    the bar the device is held to."""
    g = golden(name)
    vocoder, sr, T = str(g["vocoder"]), int(g["sr"]), int(g["T"])
    W = fold_weight_norm(synthetic.make_synth_ckpt(sr, str(g["version"]), int(g["seed"]), vocoder=vocoder)["weight"])
    upp = g["har"].shape[-1] // T
    _, phase0, sine, _ = vu.golden_draws(g, [(1, 1)] * (int(g["n_draws"]) - 3))
    phase0[:, 0] = 0
    if vocoder == "RefineGAN":
        lin_w, lin_b, linear = W["dec.m_source.merge.0.weight"].reshape(-1).tolist(), 0.0, True
    else:
        lin_w = W["dec.m_source.l_linear.weight"].reshape(-1).tolist()
        lin_b, linear = float(W["dec.m_source.l_linear.bias"]), False
    har = vu.np_harmonic_source(g["pitchf"], phase0.numpy(), sine.numpy(), upp, sr, lin_w, lin_b, linear)
    err = vu.rms(har, g["har"])
    print(name, "har rms error", err, "har_ref_spread", float(g["har_ref_spread"]))
    assert err < max(4 * float(g["har_ref_spread"]), 1e-6)


@pytest.mark.parametrize("vocoder", ["MRF-HiFi-GAN", "RefineGAN"])
def test_native_synth_refuses_the_new_vocoders(vocoder):
    """The model-level C API loads the Default decoder only: NotImplementedError naming the vocoder, raised before
    the library (or a device) is touched."""
    from rvc_amd.native import NativeSynth
    ck = synthetic.make_synth_ckpt(40000, "v2", seed=3, vocoder=vocoder)
    with pytest.raises(NotImplementedError, match=vocoder):
        NativeSynth(ck)
