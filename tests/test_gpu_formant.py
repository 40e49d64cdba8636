"""Formant shifting on the device (csrc/formant.hip, rvc_amd/formant.py) against the reference's own output
(tests/golden/formant.npz: stftpitchshift.py run by tests/golden/make_golden_formant.py) and, at a size the
fixture does not hold, the numpy restatement that tests/test_formant_cpu.py pins to it; plus the
formant_shifting wiring of load_audio and convert_audio."""
import os

import numpy as np
import pytest
import torch

import formant_ref
from rvc_amd import audio_io, formant, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "formant.npz"))
NAMES = sorted(k[4:] for k in GOLD.files if k.startswith("out_"))


def ulps(a, ref):
    return np.abs(a - ref).max() / np.spacing(np.float32(np.abs(ref).max()))


@pytest.fixture(scope="module")
def cases():
    return formant_ref.cases()


@pytest.fixture(scope="module")
def speech_out(cases):
    """The device's output for the first golden case from a numpy f32 input, shared by the interface tests."""
    x, qf, tb = cases["speech0"]
    return formant.shiftpitch(x, quefrency=qf * 1e-3, distortion=tb, device=DEV)


@pytest.mark.parametrize("name", NAMES)
def test_formant_matches_reference(cases, name):
    x, qf, tb = cases[name]
    ref = GOLD["out_" + name]
    out = formant.shiftpitch(x, factors=1, quefrency=qf * 1e-3, distortion=tb, device=DEV)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert not np.isnan(out).any()
    print(name, "ulps", ulps(out, ref))
    assert ulps(out, ref) <= 2.0  # both f64 end to end; rounding to f32 once
    tail = 1024 + 32 * ((len(x) - 1024) // 32)  # the first sample no frame reaches
    assert not ref[tail:].any() and tail + (len(x) - 1024) % 32 == len(x)
    assert not out[tail:].any()  # exact zeros


def test_formant_5s_matches_restatement():
    """M = 2469 frames: the per-frame grids, the phase walk and the overlap-add indexing past one block."""
    x = synthetic.synthetic_audio(5.0, seed=9).astype(np.float32)
    ref = formant_ref.shiftpitch(x, 0.8e-3, 0.8)
    out = formant.shiftpitch(x, quefrency=0.8e-3, distortion=0.8, device=DEV)
    assert (len(x) - 1024) // 32 + 1 == 2469 and out.shape == ref.shape and not np.isnan(out).any()
    print("5 s ulps", ulps(out, ref))
    assert ulps(out, ref) <= 2.0


def test_device_tensor_in_device_tensor_out(cases, speech_out):
    x, qf, tb = cases["speech0"]
    out = formant.shiftpitch(torch.from_numpy(x).to(DEV), quefrency=qf * 1e-3, distortion=tb, device=DEV)
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == (len(x),)
    assert torch.equal(out.cpu(), torch.from_numpy(speech_out))
    sh = formant.FormantShiftAMD(16000, 1024, 32, DEV)
    assert torch.equal(sh(torch.from_numpy(x).to(DEV), qf * 1e-3, tb), out)


def test_f64_input_returns_f64(cases, speech_out):
    x, qf, tb = cases["speech0"]
    out = formant.shiftpitch(x.astype(np.float64), quefrency=qf * 1e-3, distortion=tb, device=DEV)
    assert out.dtype == np.float64 and out.shape == speech_out.shape
    assert ulps(out, speech_out) <= 2.0


def test_two_calls_are_bit_identical(cases):
    x, qf, tb = cases["gap2"]
    sh = formant.FormantShiftAMD(16000, 1024, 32, DEV)
    xd = torch.from_numpy(x).to(DEV)
    assert torch.equal(sh(xd, qf * 1e-3, tb), sh(xd, qf * 1e-3, tb))


def test_load_audio_formant_shifting(tmp_path):
    p = str(tmp_path / "in.wav")
    audio_io.write_wav(p, synthetic.synthetic_audio(1.0, seed=14), 16000)
    got = audio_io.load_audio(p, 16000, formant_shifting=True, formant_qfrency=0.8, formant_timbre=0.8)
    want = formant.shiftpitch(audio_io.read_wav(p)[0], quefrency=0.8 * 1e-3, distortion=0.8, device=DEV)
    assert got.dtype == np.float32 and got.ndim == 1
    np.testing.assert_array_equal(got, want)
    assert np.abs(got - audio_io.load_audio(p, 16000)).max() > 1e-3


def test_convert_audio_formant_shifting(tmp_path):
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.convert import VoiceConverterAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    from rvc_amd.synth import SynthesizerAMD
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(32), DEV)
    rm = RMVPEAMD(synthetic.rmvpe_state_dict(33), DEV)
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(48000, "v2", seed=31), DEV)
    vc = VC(48000, Config(DEV), rmvpe=rm)
    src = str(tmp_path / "in.wav")
    audio_io.write_wav(src, synthetic.synthetic_audio(3.0, seed=12), 16000)
    cvt = VoiceConverterAMD(vc, net_g, hub, 48000, "v2")
    kw = dict(pitch=0, f0_method="rmvpe", index_rate=0.0, protect=0.33)
    vc.seed = 3
    plain = cvt.convert_audio(src, str(tmp_path / "plain.wav"), **kw)
    vc.seed = 3
    shifted = cvt.convert_audio(src, str(tmp_path / "shifted.wav"), formant_shifting=True, **kw)
    assert plain is not None and shifted is not None and shifted.shape == plain.shape
    assert np.abs(shifted - plain).max() > 1e-3
    # the same pipeline call on the shifted, peak-limited audio (convert.py:488-491)
    audio = formant.shiftpitch(audio_io.read_wav(src)[0], quefrency=0.8 * 1e-3, distortion=0.8, device=DEV)
    peak = np.abs(audio).max() / 0.95
    if peak > 1:
        audio /= peak
    vc.seed = 3
    want = vc.pipeline(model=hub, net_g=net_g, sid=0, audio=audio, pitch=0, f0_method="rmvpe", file_index="",
                       index_rate=0.0, pitch_guidance=1, filter_radius=3, volume_envelope=1, version="v2",
                       protect=0.33, hop_length=64, f0_autotune=False, f0_autotune_strength=1, suffix=".pth",
                       embed_suffix=".pt", f0_file=None, f0_onnx=False, pbar=None)
    np.testing.assert_array_equal(shifted, want)
