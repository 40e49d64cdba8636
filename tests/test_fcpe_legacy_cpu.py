"""fcpe-legacy f0, the parts that need no device: the restatement (tests/fcpe_legacy_ref.py) against the reference's
own output (tests/golden/fcpe_legacy*.npz, written by tests/golden/make_golden_fcpe_legacy.py), the synthetic
checkpoint's layout, the config checks, the wiring's refusal without a model and the entry points' argument
checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fcpe_legacy_ref
import fcpe_ref
from rvc_amd import _lib, fcpe_legacy, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "fcpe_legacy.npz"))
ATTN = np.load(os.path.join(HERE, "golden", "fcpe_legacy_attn.npz"))
CASES = ("a", "b", "c")
# test_fcpe_cpu.RTOL and its derivation: 20 roundings of the decoder's two 9-term sums and division on <= 9151
# cents, 4 more after
RTOL = np.log(2) / 1200 * 9151 * 20 * 2.0 ** -24 + 4 * 2.0 ** -24


def case_args(c, gold=GOLD):
    hop, p_len, thr, seed, n_layers, out_bias = gold["args_" + c]
    return dict(hop=int(hop), p_len=int(p_len), thr=float(thr),
                ckpt=dict(seed=int(seed), n_layers=int(n_layers), out_bias=float(out_bias)))


def attn_weights():
    seed, n_layers, out_bias = ATTN["args"]
    sd = synthetic.fcpe_legacy_checkpoint(seed=int(seed), n_layers=int(n_layers), out_bias=float(out_bias))["model"]
    p = "decoder._layers.0.attn."
    w = {n: sd[p + n] for n in ("to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias",
                                "to_out.weight", "to_out.bias")}
    return w, sd[p + "fast_attention.projection_matrix"]


def test_restated_attention_equals_reference():
    """One layer's SelfAttention, T = 51: in f64 the restatement gives the reference's f64 output within 1e-10; in
    f32 it is as close to it as the reference's own f32 run, within 8 x (the order of the sums differs)."""
    w, proj = attn_weights()
    x = torch.from_numpy(ATTN["x"])
    assert x.shape == (51, 512) and proj.shape == (266, 64)
    out64 = ATTN["out64"]
    got64 = fcpe_legacy_ref.self_attention(x.double(), w, proj).numpy()
    assert np.abs(got64 - out64).max() <= 1e-10
    e = float(np.abs(ATTN["out32"].astype(np.float64) - out64).max())
    got32 = fcpe_legacy_ref.self_attention(x, w, proj)
    assert got32.dtype == torch.float32
    err = float(np.abs(got32.double().numpy() - out64).max())
    print(f"f32 restatement err {err:.3e}, the reference's own {e:.3e}")
    assert 0 < e and err <= 8 * e


@pytest.mark.parametrize("c", CASES)
def test_restated_decode_equals_reference_f0(c):
    """From the reference's latents, the restated decode (no f0 range) and post give the reference's model f0 and
    final f0: in f64 from latent64 within 1e-10, and in f32 from latent32 (fcpe_ref's f32 decode, range open, and
    its post) with the same frames voiced and values within RTOL; the f64 stages alone are exact.  Every case holds
    voiced frames outside 50..1100 Hz: the clamp fcpe applies there would show."""
    a = case_args(c)
    cent = synthetic.fcpe_legacy_checkpoint(**a["ckpt"])["model"]["cent_table"].numpy()
    lat64 = np.load(os.path.join(HERE, "golden", f"fcpe_legacy_f64_{c}.npz"))["latent64"]
    got_m, got = fcpe_legacy_ref.f0_f64(lat64, cent, a["thr"], a["p_len"], a["hop"])
    np.testing.assert_array_equal(got_m > 0, GOLD["f0m64_" + c] > 0)
    np.testing.assert_allclose(got_m, GOLD["f0m64_" + c], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got, GOLD["f0_64_" + c], rtol=1e-10, atol=0)
    for lat, want_m, want in ((GOLD["latent32_" + c], GOLD["f0m32_" + c], GOLD["f0_32_" + c]),):
        f0m = fcpe_legacy_ref.decode(lat, cent, a["thr"])
        assert f0m.shape == (GOLD["x_" + c].size // 160 + 1,)
        got_m = fcpe_ref.resize(f0m, a["p_len"])
        np.testing.assert_array_equal(got_m > 0, want_m > 0)
        np.testing.assert_allclose(got_m, want_m, rtol=RTOL, atol=0)
        got = fcpe_ref.post(f0m, a["p_len"], a["hop"])
        assert got.dtype == np.float64 and got.shape == want.shape == (a["p_len"],)
        np.testing.assert_allclose(got, want, rtol=2 * RTOL, atol=0)
    np.testing.assert_array_equal(fcpe_ref.post(GOLD["f0m32_" + c], a["p_len"], a["hop"]), GOLD["f0_32_" + c])
    voiced = GOLD["f0m64_" + c] > 0
    assert 0 < voiced.sum() < voiced.size
    f0m = GOLD["f0m64_" + c][voiced]
    assert (f0m < 50).any() or (f0m > 1100).any()
    clamped = fcpe_ref.resize(fcpe_ref.decode(lat64, cent, a["thr"], 50, 1100), a["p_len"])
    assert not np.array_equal(clamped, fcpe_ref.resize(fcpe_legacy_ref.decode(lat64, cent, a["thr"]), a["p_len"]))


def test_checkpoint_layout():
    with open(os.path.join(HERE, "golden", "fcpe_legacy_keys.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    ck = synthetic.fcpe_legacy_checkpoint()
    assert len(want) == 1 + 6 + 6 * 19 + 2 + 3
    assert [(k, tuple(v.shape)) for k, v in ck["model"].items()] == want
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert ck["model"]["decoder._layers.0.attn.fast_attention.projection_matrix"].shape == (266, 64)
    f = 10 * 2 ** (ck["model"]["cent_table"].double() / 1200)
    assert abs(float(f[0]) - 32.70) < 1e-3 and abs(float(f[-1]) - 1975.5) < 0.1
    again = synthetic.fcpe_legacy_checkpoint()
    assert all(torch.equal(v, again["model"][k]) for k, v in ck["model"].items())
    other = synthetic.fcpe_legacy_checkpoint(seed=5, n_layers=1, nb_features=17)
    assert other["model"]["decoder._layers.0.attn.fast_attention.projection_matrix"].shape == (17, 64)
    assert not torch.equal(other["model"]["stack.0.weight"], ck["model"]["stack.0.weight"])


@pytest.mark.parametrize("field,edit", [
    ("out_dims", lambda c, sd: c["model"].update(out_dims=128)),
    ("input_channel", lambda c, sd: c["model"].update(input_channel=80)),
    ("confidence", lambda c, sd: c["model"].update(confidence=True)),
    ("use_input_conv", lambda c, sd: c["model"].update(use_input_conv=False)),
    ("projection_matrix", lambda c, sd: sd.update(
        {"decoder._layers.0.attn.fast_attention.projection_matrix": torch.zeros(273, 64)})),
    ("projection_matrix", lambda c, sd: sd.update(
        {"decoder._layers.0.attn.fast_attention.projection_matrix": torch.zeros(266, 32)})),
])
def test_unsupported_configs_are_named(field, edit):
    """The config is judged before any weight is touched, so this needs no device."""
    ck = synthetic.fcpe_legacy_checkpoint(n_layers=1, n_chans=8)
    edit(ck["config"], ck["model"])
    with pytest.raises(NotImplementedError, match=field):
        fcpe_legacy.FcpeLegacyAMD(ck, device="cpu")


def test_without_a_model_the_method_raises(tmp_path, monkeypatch):
    """No model given and no assets/models/predictors/fcpe_legacy.pt: "fcpe-legacy" raises naming itself and saying
    how to supply the model, alone and as a hybrid member, before anything touches a device."""
    from rvc_amd.extract import FeatureInputAMD
    monkeypatch.chdir(tmp_path)
    fi = FeatureInputAMD(device="cpu")
    x = np.zeros(16000, np.float32)
    with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy=.*fcpe_legacy.pt"):
        fi.compute_f0(x, "fcpe-legacy", 64)
    with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy="):
        fi.compute_f0(x, "hybrid[fcpe-legacy+swipe]", 64)
    assert fi._fcpe_legacy(required=False) is None


def test_performer_entry_rejects_bad_arguments():
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)  # a host pointer: every call below must return before any launch
    need = lib.rvc_performer_work_bytes(1, 8, 100, 266)
    assert need >= 8 * 272 * 65 * 4 * 2
    for bad in ((0, 8, 100, 266), (1, 0, 100, 266), (1, 8, 0, 266), (1, 8, 100, 0), (1, 8, 100, 273)):
        assert lib.rvc_performer_work_bytes(*bad) == -1
    assert lib.rvc_performer_work_bytes(1, 8, 100, 272) == lib.rvc_performer_work_bytes(1, 8, 100, 266)

    def call(D=64, M=266, T=100, work=need, q=p, ldc=0):
        return lib.rvc_performer_attention(q, p, p, p, p, 1, 8, T, D, M, ldc, 0, 0, p, work, None)

    assert call(q=None) == -22 and b"null" in lib.rvc_last_error()
    assert call(D=32) == -22 and b"D=32" in lib.rvc_last_error()
    for M in (0, 273, -1):
        assert call(M=M) == -22 and b"M=" in lib.rvc_last_error()
    assert call(T=0) == -22
    assert call(work=need - 1) == -22 and b"work" in lib.rvc_last_error()
    assert call(ldc=99) == -22 and b"stride" in lib.rvc_last_error()
    assert not buf.any()
