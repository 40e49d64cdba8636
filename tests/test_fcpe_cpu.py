"""fcpe f0, the parts that need no device: the numpy restatement (tests/fcpe_ref.py) against the reference's own
output (tests/golden/fcpe.npz, written by tests/golden/make_golden_fcpe.py), the synthetic checkpoint's layout,
the Slaney mel basis, the hybrid[...] parser's ``extra`` members, the config checks and the entry points'
argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fcpe_ref
from rvc_amd import _lib, f0mix, fcpe, melbasis, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "fcpe.npz"))
CASES = ("a", "b", "c")
# The decoder's cents = sum(c * y) / sum(y) in f32: two 9-term sums (at most 9 roundings each) and a division, so
# at most ~20 * 2^-24 relative on at most 9151 cents (f0_max 1975.5 Hz); f0 = 10 * 2^(cents / 1200) turns an error
# d in cents into ln(2) / 1200 * d relative.  The division by 1200, pow and the product add 4 more roundings.
RTOL = np.log(2) / 1200 * 9151 * 20 * 2.0 ** -24 + 4 * 2.0 ** -24


def case_args(c):
    hop, p_len, thr, f0_min, f0_max, seed, n_layers, harm = GOLD["args_" + c]
    return dict(hop=int(hop), p_len=int(p_len), thr=float(thr), f0_min=int(f0_min), f0_max=int(f0_max),
                ckpt=dict(seed=int(seed), n_layers=int(n_layers), use_harmonic_emb=bool(harm)))


@pytest.mark.parametrize("c", CASES)
def test_restatement_equals_reference_f0(c):
    """From the reference's f32 latent, fcpe_ref gives the reference's model f0 and final f0: the same frames
    voiced, the values within RTOL (the order of the decoder's two 9-term f32 sums is torch's own, and its pow is
    not numpy's exp2); the f64 stages are exact."""
    a = case_args(c)
    cent = synthetic.fcpe_checkpoint(**a["ckpt"])["model"]["cent_table"].numpy()
    lat = GOLD["latent32_" + c]
    f0m = fcpe_ref.decode(lat, cent, a["thr"], a["f0_min"], a["f0_max"])
    assert f0m.shape == (GOLD["x_" + c].size // 160 + 1,)
    got_m = fcpe_ref.resize(f0m, a["p_len"])
    want_m, want = GOLD["f0m32_" + c], GOLD["f0_32_" + c]
    np.testing.assert_array_equal(got_m > 0, want_m > 0)
    np.testing.assert_allclose(got_m, want_m, rtol=RTOL, atol=0)
    got = fcpe_ref.post(f0m, a["p_len"], a["hop"])
    assert got.dtype == np.float64 and got.shape == want.shape == (a["p_len"],)
    np.testing.assert_allclose(got, want, rtol=2 * RTOL, atol=0)
    # the f64 stages alone, from the reference's own model f0: exact
    np.testing.assert_array_equal(fcpe_ref.post(want_m, a["p_len"], a["hop"]), want)
    voiced = want_m > 0
    assert 0 < voiced.sum() < voiced.size


def test_resize_matches_torch():
    """fcpe_ref.resize against F.interpolate itself, bit for bit, NaN pattern included."""
    rng = np.random.default_rng(3)
    for T in (2, 7, 50, 151, 300):
        for P in sorted({T - 1, T, 2 * T + 3, max(T // 2, 1), T + 1}):
            x = (rng.random(T) * 900 + 60).astype(np.float32)
            x[rng.random(T) < 0.35] = 0
            t = torch.from_numpy(x)[None, None]
            want = torch.nn.functional.interpolate(torch.where(t == 0, float("nan"), t), size=P, mode="linear")
            want = torch.where(want.isnan(), 0.0, want)[0, 0].numpy()
            np.testing.assert_array_equal(fcpe_ref.resize(x, P), want, err_msg=f"T={T} P={P}")


def test_checkpoint_layout():
    with open(os.path.join(HERE, "golden", "fcpe_keys.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    ck = synthetic.fcpe_checkpoint()
    assert len(want) == 73
    assert [(k, tuple(v.shape)) for k, v in ck["model"].items()] == want
    assert all(v.dtype == torch.float32 for v in ck["model"].values())
    assert ck["config_dict"]["model"]["conv_only"] is True and ck["config_dict"]["mel"]["sr"] == 16000
    again = synthetic.fcpe_checkpoint()
    assert all(torch.equal(v, again["model"][k]) for k, v in ck["model"].items())
    small = synthetic.fcpe_checkpoint(seed=5, n_layers=2, hidden_dims=64, use_harmonic_emb=True)
    assert small["model"]["harmonic_emb.weight"].shape == (9, 64)
    assert len(small["model"]) == 2 + 1 + 6 + 2 * 10 + 5


def test_slaney_basis():
    """The Slaney-scale basis (librosa's defaults): Slaney's area norm makes every filter a triangle of unit area
    over Hz, so its peak is at most 2 / (its band's width) and its bins sum to about 1 / (bin spacing); the
    filters are centred in increasing order; the HTK form is bit-identical to what RMVPE has always been given."""
    sr, n_fft, n_mels = 16000, 1024, 128
    B = melbasis.mel_filterbank(sr, n_fft, n_mels, 0, 8000, htk=False)
    assert B.shape == (128, 513) and B.dtype == np.float32 and (B >= 0).all()
    edges = melbasis.mel_to_hz_slaney(np.linspace(0, melbasis.hz_to_mel_slaney(8000.0)[0], n_mels + 2))
    np.testing.assert_allclose(edges[:4], np.arange(4) * edges[1], rtol=1e-12)  # linear below 1 kHz
    np.testing.assert_allclose(edges[-1], 8000.0, rtol=1e-12)
    width = edges[2:] - edges[:-2]
    assert (B.max(axis=1) <= 2.0 / width * (1 + 1e-6)).all()
    df = sr / n_fft
    wide = width > 8 * df  # enough bins under the triangle for the sum to approximate its area
    assert wide.sum() > 40
    np.testing.assert_allclose(B[wide].sum(axis=1) * df, 1.0, rtol=0.05)
    assert (np.diff(B.argmax(axis=1)) >= 0).all()
    # every filter is zero outside its band
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    for m in (0, 17, 64, 127):
        outside = (freqs <= edges[m]) | (freqs >= edges[m + 2])
        assert not B[m][outside].any()
    # htk=True is the old function, bit for bit (the default, and the values RMVPE's golden vectors pin)
    old = melbasis.mel_filterbank(16000, 1024, 128, 30.0, 8000.0)
    assert old.tobytes() == melbasis.mel_filterbank(16000, 1024, 128, 30.0, 8000.0, htk=True).tobytes()
    mel_f = melbasis.mel_to_hz_htk(np.linspace(melbasis.hz_to_mel_htk(30.0), melbasis.hz_to_mel_htk(8000.0), 130))
    ramps = np.subtract.outer(mel_f, freqs)
    want = np.zeros((128, 513), np.float32)
    for i in range(128):
        want[i] = np.maximum(0, np.minimum(-ramps[i] / np.diff(mel_f)[i], ramps[i + 2] / np.diff(mel_f)[i + 1]))
    want *= (2.0 / (mel_f[2:130] - mel_f[:128]))[:, np.newaxis]
    assert old.tobytes() == want.tobytes()
    assert not np.array_equal(old, melbasis.mel_filterbank(16000, 1024, 128, 30.0, 8000.0, htk=False))


def test_hybrid_parser_extra_members():
    assert f0mix.parse_hybrid("hybrid[fcpe+swipe]", extra=("fcpe",)) == ["fcpe", "swipe"]
    with pytest.raises(NotImplementedError, match="fcpe"):
        f0mix.parse_hybrid("hybrid[fcpe+swipe]")
    for extra in ((), ("fcpe",)):
        with pytest.raises(NotImplementedError, match="fcpe-legacy"):
            f0mix.parse_hybrid("hybrid[fcpe-legacy+swipe]", extra=extra)
        with pytest.raises(NotImplementedError, match="harvest"):
            f0mix.parse_hybrid("hybrid[swipe+harvest]", extra=extra)
    assert "fcpe" not in f0mix.MEMBERS


@pytest.mark.parametrize("field,edit", [
    ("conv_only", lambda c: c["model"].update(conv_only=False)),
    ("mel.type", lambda c: c["mel"].update(type="stft")),
    ("mel.sr", lambda c: c["mel"].update(sr=44100)),
    ("mel.hop_size", lambda c: c["mel"].update(hop_size=256)),
    ("mel.num_mels", lambda c: c["mel"].update(num_mels=80)),
    ("mel.fmax", lambda c: c["mel"].update(fmax=7600)),
])
def test_unsupported_configs_are_named(field, edit):
    """The config is judged before any weight is touched, so this needs no device."""
    ck = synthetic.fcpe_checkpoint(n_layers=1, hidden_dims=8)
    edit(ck["config_dict"])
    with pytest.raises(NotImplementedError, match=field.replace(".", r"\.")):
        fcpe.FcpeAMD(ck, device="cpu")


def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    buf = np.zeros(4096, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)  # a host pointer: every call below must return before any launch
    assert lib.rvc_fcpe_mel(None, None, None, 1, 16000, None) == -22
    assert b"null" in lib.rvc_last_error()
    assert lib.rvc_fcpe_mel(p, p, p, 1, 432, None) == -22
    assert b"constant-padding" in lib.rvc_last_error()
    assert lib.rvc_fcpe_mel(p, p, p, 0, 16000, None) == -22
    assert lib.rvc_groupnorm_work_bytes(1, 4) > 0 and lib.rvc_groupnorm_work_bytes(0, 4) == -1
    assert lib.rvc_groupnorm_act(None, None, None, None, 1, 8, 4, 4, 1e-5, 0.01, None, 0, None) == -22
    assert lib.rvc_groupnorm_act(p, p, p, p, 1, 10, 4, 4, 1e-5, 0.01, p, 1 << 20, None) == -22
    assert b"groups" in lib.rvc_last_error()
    assert lib.rvc_groupnorm_act(p, p, p, p, 1, 8, 0, 4, 1e-5, 0.01, p, 1 << 20, None) == -22
    assert lib.rvc_groupnorm_act(p, p, p, p, 1, 8, 4, 4, 1e-5, 0.01, p, 8, None) == -22
    assert b"work" in lib.rvc_last_error()
    assert lib.rvc_glu_dwconv_silu(None, None, None, None, 1, 8, 16, 31, None) == -22
    for K in (0, 4, 33):
        assert lib.rvc_glu_dwconv_silu(p, p, p, ctypes.c_void_p(buf.ctypes.data + 64), 1, 8, 16, K, None) == -22
        assert b"K=" in lib.rvc_last_error()
    assert lib.rvc_glu_dwconv_silu(p, p, p, p, 1, 8, 16, 31, None) == -22  # in place
    assert lib.rvc_glu_dwconv_silu(p, p, p, ctypes.c_void_p(buf.ctypes.data + 64), 1, 8, 0, 31, None) == -22
    assert lib.rvc_fcpe_decode(None, None, None, 1, 360, 10, 0.006, 50.0, 1100.0, None) == -22
    assert lib.rvc_fcpe_decode(p, p, p, 1, 0, 10, 0.006, 50.0, 1100.0, None) == -22
    assert lib.rvc_fcpe_decode(p, p, p, 1, 360, 10, 0.006, 1100.0, 50.0, None) == -22
    assert b"f0_min" in lib.rvc_last_error()
    assert lib.rvc_fcpe_post_work_bytes(150) >= 150 * 12
    assert lib.rvc_fcpe_post_work_bytes(0) == -1 and lib.rvc_fcpe_post_work_bytes(1 << 24) == -1
    assert lib.rvc_fcpe_post(None, 10, 10, 160, 16000, None, 0, None, None) == -22
    assert lib.rvc_fcpe_post(p, 0, 10, 160, 16000, p, 1 << 20, p, None) == -22
    assert lib.rvc_fcpe_post(p, 10, 0, 160, 16000, p, 1 << 20, p, None) == -22
    assert lib.rvc_fcpe_post(p, 10, 10, 0, 16000, p, 1 << 20, p, None) == -22
    assert b"hop_length" in lib.rvc_last_error()
    assert lib.rvc_fcpe_post(p, 10, 10, 160, 16000, p, 8, p, None) == -22
    assert b"work" in lib.rvc_last_error()
    assert not buf.any()
