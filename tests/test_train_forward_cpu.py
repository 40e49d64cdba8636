"""CPU-side checks of the training forward (rvc_amd.train_forward): the f64 restatement tests/train_forward_ref.py
against the reference's own f64 stages (tests/golden/train_forward_*.npz, made by
tests/golden/make_golden_train_forward.py), the checkpoint key mapping, the experiment-folder parsing and
aggregation arithmetic, and the refusals.  Nothing here touches a device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import train_forward_ref as ref
from conftest import GOLDEN
from rvc_amd import _lib, synthetic, train_forward as tf

CASES = {"a": (40000, "v2"), "b": (48000, "v2"), "c": (32000, "v1")}
# the restatement and the reference's f64 run are the same arithmetic in another order: f64 rounding times the
# depth of the sums (2048-point FFTs, 1025-term dot products, 16-layer stacks), far below any f32 figure
F64_TOL = 1e-11


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request, golden):
    name = request.param
    sr, version = CASES[name]
    fx = golden(f"train_forward_{name}")
    fx["spec_f64"] = golden(f"train_forward_{name}_spec")["spec_f64"]
    hps = synthetic.train_config(sr, version)
    W = ref.fold64(ref.fixture_ckpt(fx, sr, version)["model"])
    return name, fx, hps, W


def test_fixture_shapes_and_slice(case):
    name, fx, hps, _ = case
    d = hps["data"]
    T, S = int(fx["T"]), int(fx["S"])
    assert S == hps["train"]["segment_size"] // d["hop_length"]
    assert fx["spec_f64"].shape == (1, d["filter_length"] // 2 + 1, T)
    assert fx["wav"].shape == (1, T * d["hop_length"])
    start = int(fx["ids_slice"][0])
    # commons.py:31: the f32 product truncated
    assert start == int(np.float32(fx["slice_u"][0]) * np.float32(T - S + 1))
    assert (start > 0) if name == "b" else True
    assert (start == 0 and T == S) if name == "c" else True
    assert 0.15 < float(np.mean(fx["pitchf"] == 0)) < 0.4  # about a quarter of the frames unvoiced


def test_restated_spectrogram_and_mels(case):
    _, fx, hps, _ = case
    d = hps["data"]
    n_fft, hop, S = d["filter_length"], d["hop_length"], int(fx["S"])
    spec = ref.spectrogram(fx["wav"], n_fft, hop)
    assert _rel(spec, fx["spec_f64"]) < F64_TOL
    basis = ref.mel_basis(d["sample_rate"], n_fft, d["n_mel_channels"], d["mel_fmin"], d["mel_fmax"])
    mel = ref.mel_log(fx["spec_f64"], basis)
    y_mel = ref.slice_segments(mel, fx["ids_slice"], S)
    assert _rel(y_mel, fx["y_mel_f64"]) < F64_TOL
    y_hat_mel = ref.mel_log(ref.spectrogram(fx["y_hat_f64"].reshape(1, -1), n_fft, hop), basis)
    assert _rel(y_hat_mel, fx["y_hat_mel_f64"]) < 1e-9  # log of small band energies amplifies the last bits
    l1 = ref.slice_l1(mel, fx["ids_slice"], fx["y_hat_mel_f64"])
    assert abs(l1 * hps["train"]["c_mel"] / float(fx["loss_mel_f64"]) - 1) < F64_TOL


def test_restated_posterior_flow_and_kl(case):
    _, fx, hps, W = case
    g = ref.speaker(W, fx["sid"][0])
    z, m_q, logs_q = ref.posterior(W, torch.from_numpy(fx["spec_f64"]), g, fx["z_noise"])
    for got, key in ((z, "z"), (m_q, "m_q"), (logs_q, "logs_q")):
        assert _rel(got, fx[key + "_f64"]) < F64_TOL, key
    z_p = ref.flow_forward(W, fx["z_f64"], g)
    assert _rel(z_p, fx["z_p_f64"]) < F64_TOL
    # m_p / logs_p: the prior encoder, pinned by the synthesizer fixtures, here through the oracle in f64
    from oracle import synth as osy
    T = int(fx["T"])
    torch.set_default_dtype(torch.float64)  # the oracle allocates its scratch in the default dtype
    try:
        m_p, logs_p, _ = osy.text_encoder(W, tf.config_list(hps), torch.from_numpy(fx["phone"]).double(),
                                          torch.from_numpy(fx["pitch"]), torch.tensor([T]))
    finally:
        torch.set_default_dtype(torch.float32)
    kl = ref.kl_loss(fx["z_p_f64"], fx["logs_q_f64"], m_p, logs_p)
    # kl_loss casts its operands with .float() (train.py:318-322), so the reference's f64 run still sums the KL in
    # f32: one f32 rounding per term and torch's pairwise sum over 192 * T of them, about log2(n) = 13 roundings deep
    assert abs(kl * hps["train"]["c_kl"] / float(fx["loss_kl_f64"]) - 1) < 13 * 2.0 ** -24


def test_reference_f32_sits_where_the_fixture_says(case):
    """ref_dev: the reference f32's distance from its f64, the scale the device figures are read against."""
    _, fx, _, _ = case
    dev = dict(zip([str(s) for s in fx["ref_dev_stages"]], fx["ref_dev"]))
    assert set(dev) == {"spec", "m_q", "logs_q", "z", "z_p", "y_hat", "y_mel", "y_hat_mel"}
    for k, (rms, mx, ref_rms, ref_max) in dev.items():
        assert 0 < rms <= mx and rms / ref_rms < 1e-5, k
    assert abs(float(fx["loss_mel_f32"]) / float(fx["loss_mel_f64"]) - 1) < 1e-5
    assert abs(float(fx["loss_kl_f32"]) / float(fx["loss_kl_f64"]) - 1) < 1e-5


# ---------------------------------------------------------------------- checkpoint layout
def test_enc_q_key_mapping_covers_reference_state_dict():
    """The loader reads exactly the keys of the reference enc_q's own state_dict() (tests/golden/enc_q_keys.json, in
    save_checkpoint's naming), and the synthetic weights have the reference's shapes."""
    table = json.load(open(os.path.join(GOLDEN, "enc_q_keys.json")))["32000/v1"]
    assert sorted(tf.enc_q_keys()) == sorted(table)
    cfg = synthetic.synth_config(32000, "v1")
    sd = synthetic.enc_q_state_dict(cfg, 7)
    assert {k: list(v.shape) for k, v in sd.items()} == table
    # the wider spectrogram of the 2048-point configs only widens the pre conv
    sd40 = synthetic.enc_q_state_dict(synthetic.synth_config(40000, "v2"), 7)
    assert sd40["enc_q.pre.weight"].shape == (192, 1025, 1)
    assert {k: v.shape for k, v in sd40.items() if k != "enc_q.pre.weight"} == \
        {k: v.shape for k, v in sd.items() if k != "enc_q.pre.weight"}


def test_train_ckpt_wraps_synth_weights_unchanged():
    ck = synthetic.make_train_ckpt(40000, "v2", seed=11)
    assert set(ck) >= {"model", "iteration", "optimizer", "learning_rate"}
    plain = synthetic.synth_state_dict(synthetic.synth_config(40000, "v2"), 11)
    assert [k for k in ck["model"] if not k.startswith("enc_q.")] == list(plain)
    for k, v in plain.items():
        assert torch.equal(ck["model"][k], v), k
    assert tf.config_list(synthetic.train_config(48000, "v2"))[:2] == [1025, 36]
    assert tf.config_list(synthetic.train_config(32000, "v1"))[:2] == [513, 40]


def test_refusals_by_name():
    hps = synthetic.train_config(40000, "v2")
    model = synthetic.make_train_ckpt(40000, "v2", seed=3)["model"]
    tf.check_supported(model, hps)
    drop = json.loads(json.dumps(hps))
    drop["model"]["p_dropout"] = 0.1
    with pytest.raises(NotImplementedError, match="p_dropout"):
        tf.TrainSynthAMD({"model": model}, drop, device="cpu")
    with pytest.raises(NotImplementedError, match="no-f0"):
        tf.TrainSynthAMD({"model": model}, hps, device="cpu", f0=False)
    nof0 = {k: v for k, v in model.items() if k != "enc_p.emb_pitch.weight"}
    with pytest.raises(NotImplementedError, match="no-f0"):
        tf.TrainSynthAMD({"model": nof0}, hps, device="cpu")
    for voc in ("MRF-HiFi-GAN", "RefineGAN"):
        with pytest.raises(NotImplementedError, match=voc):
            tf.TrainSynthAMD({"model": model}, hps, device="cpu", vocoder=voc)
    infer_only = {k: v for k, v in model.items() if not k.startswith("enc_q.")}
    with pytest.raises(KeyError, match="enc_q"):
        tf.TrainSynthAMD({"model": infer_only}, hps, device="cpu")


# ---------------------------------------------------------------------- experiment folders
def test_filelist_parse_and_length_trim(tmp_path):
    fl = tmp_path / "filelist.txt"
    fl.write_text("a/0.wav|a/0.npy|b/0.npy|c/0.npy|0\n\nx y/1.wav|p|q|r|spk\n")
    rows = tf.read_filelist(str(fl))
    assert rows == [("a/0.wav", "a/0.npy", "b/0.npy", "c/0.npy", "0"), ("x y/1.wav", "p", "q", "r", "spk")]
    assert [tf.parse_sid(r[4]) for r in rows] == [0, 0] and tf.parse_sid("17") == 17
    fl.write_text("a.wav|b|c\n")
    with pytest.raises(ValueError, match="expected wav"):
        tf.read_filelist(str(fl))
    # phone frames x2; pitch arrays as long as the doubled phone; the spectrogram one frame shorter
    phone = np.arange(30 * 4, dtype=np.float32).reshape(30, 4)
    pitch, pitchf = np.arange(60), np.arange(60, dtype=np.float32)
    p, c, f, T = tf.trim_labels(phone, pitch, pitchf, 59)
    assert T == 59 and p.shape == (59, 4) and len(c) == 59 and len(f) == 59
    assert np.array_equal(p[:4], phone[[0, 0, 1, 1]])
    # the 900-frame cap, then a longer spectrogram cuts nothing more
    phone = np.zeros((500, 2), np.float32)
    p, c, f, T = tf.trim_labels(phone, np.arange(1000), np.arange(1000.0), 950)
    assert T == 900 and p.shape == (900, 2) and c[-1] == 899 and f[-1] == 899.0
    # phone shorter than the spectrogram
    p, c, f, T = tf.trim_labels(np.zeros((10, 2), np.float32), np.arange(25), np.arange(25.0), 24)
    assert T == 20 and len(c) == 20


def test_aggregate_is_what_a_reference_batch_logs():
    """Against the reference's own formulas on a made-up padded batch: l1_loss over equal slices, kl_loss's summed KL
    over the summed mask (train.py:317-325, 865-866)."""
    rng = np.random.default_rng(5)
    frames = [40, 57, 33]
    c_mel, c_kl = 45, 1.0
    l1 = [float(rng.uniform(1, 4)) for _ in frames]                  # each utterance's slice mean
    kl_sum = [float(rng.uniform(50, 90)) * T for T in frames]        # each utterance's summed KL
    per = [{"loss_mel": c_mel * a, "loss_kl": c_kl * s / T, "frames": T} for a, s, T in zip(l1, kl_sum, frames)]
    got = tf.aggregate(per)
    assert got["loss_mel"] == pytest.approx(c_mel * np.mean(l1), rel=1e-12)
    assert got["loss_kl"] == pytest.approx(c_kl * sum(kl_sum) / sum(frames), rel=1e-12)
    assert got["loss_kl"] != pytest.approx(np.mean([p["loss_kl"] for p in per]), rel=1e-6)
    assert tf.aggregate([]) == {"loss_mel": None, "loss_kl": None}


def test_ops_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    assert lib.rvc_spectrogram_frames(19200, 2048, 400) == 48
    assert lib.rvc_spectrogram_frames(12800, 1024, 320) == 40
    assert lib.rvc_spectrogram_frames(825, 2048, 400) == 2      # barely longer than the reflect pad of 824
    assert lib.rvc_spectrogram_frames(824, 2048, 400) == -1     # the pad does not fit
    assert lib.rvc_spectrogram_frames(4000, 1024, 321) == -1    # n_fft - hop odd
    assert lib.rvc_spectrogram(None, None, None, 1, 19200, 48, 2048, 400, None) == -22
    assert lib.rvc_spectrogram(p, p, p, 1, 19200, 48, 4096, 400, None) == -22
    assert b"1024 or 2048" in lib.rvc_last_error()
    assert lib.rvc_spectrogram(p, p, p, 1, 19200, 47, 2048, 400, None) == -22
    assert lib.rvc_mel_log(p, p, p, 1, 0, 1025, 48, None) == -22
    nb = lib.rvc_trainfwd_work_bytes()
    assert nb == 64 * 8
    assert lib.rvc_slice_l1(p, p, p, 1, 125, 30, 32, p, nb, p, None) == -22      # S > T
    assert lib.rvc_slice_l1(p, p, p, 1, 125, 48, 32, p, nb - 1, p, None) == -22  # short work buffer
    assert lib.rvc_kl_loss(p, p, p, None, 1, 192, 48, 0, 0, p, nb, p, None) == -22
    assert lib.rvc_kl_loss(p, p, p, p, 2, 192, 48, 0, 100, p, nb, p, None) == -22
