"""Formant shifting, the parts that need no device: the numpy restatement (tests/formant_ref.py) against
the reference's own output (tests/golden/formant.npz, written by tests/golden/make_golden_formant.py), the
C ABI's argument checks, the Python front end's refusals and load_audio's unchanged default path."""
import ctypes
import os

import numpy as np
import pytest

import formant_ref
from rvc_amd import _lib, audio_io, formant, synthetic

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "formant.npz"))
NAMES = sorted(k[4:] for k in GOLD.files if k.startswith("out_"))


def ulps(a, ref):
    return np.abs(a - ref).max() / np.spacing(np.float32(np.abs(ref).max()))


@pytest.fixture(scope="module")
def cases():
    return formant_ref.cases()


def test_fixture_holds_every_case(cases):
    assert NAMES == sorted(cases) and len(NAMES) == 14
    for name, (x, qf, tb) in cases.items():
        assert tuple(GOLD["par_" + name]) == (qf, tb)
        assert GOLD["out_" + name].shape == x.shape and GOLD["out_" + name].dtype == np.float32


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(cases, name):
    """The vectorised restatement is within the device's own bound of the reference on every golden case."""
    x, qf, tb = cases[name]
    ref = GOLD["out_" + name]
    out = formant_ref.shiftpitch(x, qf * 1e-3, tb)
    assert out.dtype == np.float32 and out.shape == ref.shape and not np.isnan(out).any()
    assert ulps(out, ref) <= 2.0
    tail = 1024 + 32 * ((len(x) - 1024) // 32)  # the first sample no frame reaches
    assert not ref[tail:].any() and not out[tail:].any()


def formant_args(**kw):
    a = _lib.FormantArgs()
    a.n_fft, a.hop, a.sample_rate, a.quefrency_samples, a.distortion = 1024, 32, 16000, 12, 0.8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_rejects_bad_args_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: every call below is refused before a launch
    a = formant_args()
    assert lib.rvc_formant_work_bytes(24000, ctypes.byref(a)) > 0
    assert lib.rvc_formant_work_bytes(24000, None) == -1
    assert lib.rvc_formant_shift(None, 24000, ctypes.byref(a), None, 0, None, None) == -22
    assert b"null" in lib.rvc_last_error()
    assert lib.rvc_formant_shift(one, 24000, None, one, 1 << 40, one, None) == -22
    assert b"null" in lib.rvc_last_error()
    a.window = a.synth_window = one
    for n, bad, word in ((1023, {}, b"shorter"), (24000, {"quefrency_samples": 513}, b"quefrency"),
                         (24000, {"quefrency_samples": -1}, b"quefrency"), (24000, {"distortion": 0.0}, b"distortion"),
                         (24000, {"distortion": -1.0}, b"distortion"), (24000, {"distortion": float("nan")}, b"distortion"),
                         (24000, {"distortion": float("inf")}, b"distortion"), (24000, {"n_fft": 1000}, b"n_fft")):
        b = formant_args(window=one, synth_window=one, **bad)
        assert lib.rvc_formant_shift(one, n, ctypes.byref(b), one, 1 << 40, one, None) == -22, (n, bad)
        assert word in lib.rvc_last_error(), (n, bad, lib.rvc_last_error())
        assert lib.rvc_formant_work_bytes(n, ctypes.byref(b)) == -1
    # a work buffer that is too small is refused too
    assert lib.rvc_formant_shift(one, 24000, ctypes.byref(a), one, 16, one, None) == -22
    assert b"work" in lib.rvc_last_error()


def test_front_end_refusals_need_no_device():
    x = synthetic.synthetic_audio(0.2, seed=1)
    with pytest.raises(NotImplementedError):
        formant.shiftpitch(x, factors=2)
    with pytest.raises(NotImplementedError):
        formant.shiftpitch(x, factors=[1, 1.5])
    with pytest.raises(NotImplementedError):
        formant.shiftpitch(x, normalization=True)
    with pytest.raises(NotImplementedError):
        formant.shiftpitch((x * 32767).astype(np.int16))
    with pytest.raises(NotImplementedError):
        formant.shiftpitch(x, framesize=(1024, 512))
    with pytest.raises(ValueError):
        formant.shiftpitch(x[:1023], quefrency=0.8e-3, distortion=0.8)
    with pytest.raises(ValueError):
        formant.shiftpitch(np.stack([x, x]))


def test_load_audio_default_path_is_unchanged(tmp_path):
    """Without the flag load_audio does not touch the shifter: the file's samples, as before."""
    p = str(tmp_path / "a.wav")
    audio_io.write_wav(p, synthetic.synthetic_audio(0.3, seed=2), 16000)
    want = audio_io.read_wav(p)[0]
    for got in (audio_io.load_audio(p), audio_io.load_audio(p, 16000), audio_io.load_audio(p, 16000, False, 0.8, 0.8)):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
    # a file shorter than one frame: the shifter's ValueError comes back as RuntimeError, before any device call
    q = str(tmp_path / "short.wav")
    audio_io.write_wav(q, synthetic.synthetic_audio(0.05, seed=2), 16000)
    with pytest.raises(RuntimeError):
        audio_io.load_audio(q, 16000, formant_shifting=True)
