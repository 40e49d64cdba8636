"""CPU-side checks of dataset preprocessing: the numpy / scipy restatement (tests/preprocess_ref.py) against the
reference's own output (tests/golden/preprocess*.npz, written by tests/golden/make_golden_preprocess.py), the chunk
planner at its edges, the lfilter warm-up rule, and the new C entries (present, and refusing bad arguments before
any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import signal

import preprocess_ref as R
from rvc_amd import _lib, audio_io, synthetic
from rvc_amd import preprocess as pre

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = [(0.3, 0), (2.0, 1), (0.6, 0), (1.7, 1), (0.2, 0)]
SYMBOLS = ["rvc_lfilter64_warmup", "rvc_lfilter64_work_bytes", "rvc_lfilter64", "rvc_frame_rms64_len",
           "rvc_frame_rms64", "rvc_peak_mix64", "rvc_resample_poly64"]


def load_fixture(golden):
    g = golden("preprocess")
    gt = {**golden("preprocess_gt_a"), **golden("preprocess_gt_b")}
    k16 = golden("preprocess_16k")
    n = len(g["names"])
    g["gt"] = [gt[f"gt_{k}"] for k in range(n)]
    g["k16"] = [k16[f"k16_{k}"] for k in range(n)]
    return g


def test_restatement_matches_reference(golden):
    g = load_fixture(golden)
    sr, per, seed = int(g["args"][0]), float(g["args"][1]), int(g["args"][2])
    audio = synthetic.silence_layout_audio(LAYOUT, seed=seed, sr=sr)
    out = R.chain(audio, sr, per)
    assert [f"0_0_{k}.wav" for k in range(len(out["gt"]))] == list(g["names"])
    assert np.array_equal(out["offsets"], g["offsets"])
    assert [[len(a), len(b)] for a, b in zip(out["gt"], out["k16"])] == g["lengths"].tolist()
    assert g["lengths"][:, 0].tolist() == [32000, 32000, 38720, 32000, 32000, 25280]
    assert np.array_equal(out["rms"], g["rms"]) and np.abs(g["rms"] / g["threshold"] - 1).min() >= 0.09
    for k in range(len(out["gt"])):
        assert out["gt"][k].dtype == np.float32 and out["k16"][k].dtype == np.float32
        assert np.abs(out["gt"][k].astype(np.float64) - g["gt"][k]).max() <= g["tol_gt"]
        assert np.abs(out["k16"][k].astype(np.float64) - g["k16"][k]).max() <= g["tol_16k"]
    # the sosfilt form of the chain is the yardstick the tolerances come from: it sits inside them too
    sos = R.chain(audio, sr, per, filt="sosfilt")
    assert np.array_equal(sos["offsets"], g["offsets"])
    d = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(sos["gt"], g["gt"]))
    assert 0 < d <= g["tol_gt"] / 2


@pytest.mark.parametrize("plan", [R.plan_chunks, pre.plan_chunks], ids=["ref", "amd"])
def test_chunk_planner_edges(plan):
    sr, per = 32000, 1.0
    edge = int((per + R.OVERLAP) * sr)
    assert edge == 41600 and (per + R.OVERLAP) * sr == 41600.0
    assert plan(edge, sr, per) == [(0, edge)]  # strict >: exactly (per + OVERLAP) * sr stays one chunk
    assert plan(edge + 1, sr, per) == [(0, 32000), (22400, edge + 1 - 22400)]
    assert plan(0, sr, per) == [(0, 0)]
    assert plan(5, sr, per) == [(0, 5)]
    # sr * (per - OVERLAP) * i is 12799.999..., 25599.999..., ... in f64: int() truncates each to one sample early
    sr, per = 32000, 0.7
    hop = [int(sr * (per - R.OVERLAP) * i) for i in range(4)]
    assert int(per * sr) == 22400 and hop == [0, 12799, 25599, 38399]
    n = 100000
    got = plan(n, sr, per)
    want, i = [], 0
    while True:  # preprocess.py:171-182 on a list of indices
        seg = list(range(n))[int(sr * (per - R.OVERLAP) * i):]
        i += 1
        if len(seg) > (per + R.OVERLAP) * sr:
            want.append((seg[0], len(seg[: int(per * sr)])))
        else:
            want.append((seg[0], len(seg)))
            break
    assert got == want and len(got) > 3
    # a non-integer per * sr: the chunk length is its truncation
    sr, per = 40000, 0.37777
    assert per * sr != int(per * sr)
    got = plan(90000, sr, per)
    assert all(ln == int(per * sr) for _, ln in got[:-1]) and got[1][0] == int(sr * (per - R.OVERLAP))
    assert got[-1][0] + got[-1][1] == 90000 and got[-1][1] <= (per + R.OVERLAP) * sr


@pytest.mark.parametrize("sr,measured", [(16000, 3973), (32000, 7848), (40000, 9503), (48000, 11383)])
def test_warmup_rule(sr, measured):
    """The decay measured for the 48 Hz Butterworth and the rule the library derives from b, a."""
    b, a = signal.butter(N=5, Wn=48, btype="high", fs=sr)
    warm = pre.warmup(b, a)
    tile = _lib.LFILTER_TILE
    assert warm % tile == 0 and measured < warm <= measured + tile
    assert warm == R.warmup_rule(b, a, tile) and warm <= _lib.LFILTER_WARM_CAP
    assert warm > 3584 or sr == 16000  # the 16 kHz constant of filtfilt.hip does not carry over


def test_warmup_rejects_slow_filters():
    b, a = signal.butter(N=5, Wn=48, btype="high", fs=96000)  # needs ~21.7k samples
    assert R.warmup_rule(b, a) > _lib.LFILTER_WARM_CAP
    with pytest.raises(ValueError):
        pre.warmup(b, a)
    with pytest.raises(ValueError):
        pre.warmup(b, np.array([1.0, -2.5, 0, 0, 0, 0]))  # unstable: never decays
    with pytest.raises(ValueError):
        pre.warmup(b[:5], a[:5])


def test_chunked_recurrence_is_within_the_ba_forms_noise():
    """The device lfilter's arithmetic, restated in numpy: chunks that reach n = 0 are scipy's bits, the others sit
    within twice the difference between scipy's own two forms of the filter (the GPU test's tolerance)."""
    sr, n = 48000, 60000
    b, a = signal.butter(N=5, Wn=48, btype="high", fs=sr)
    sos = signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos")
    rng = np.random.default_rng(11)
    t = np.arange(n) / sr
    x = (0.3 + 0.4 * np.sin(2 * np.pi * 30 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    ref = signal.lfilter(b, a, x)
    e = np.abs(ref - signal.sosfilt(sos, x.astype(np.float64))).max()
    warm = R.warmup_rule(b, a)
    y = R.lfilter_chunked(b, a, x, warm)
    assert np.array_equal(y[:512], ref[:512])
    assert np.abs(y - ref).max() <= max(2 * e, 1e-12)
    short = R.lfilter_chunked(b, a, x, 3584)  # filtfilt.hip's 16 kHz warm-up leaks DC and 30 Hz at 48 kHz
    assert np.abs(short - ref).max() > 1e-4


def test_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert set(SYMBOLS) <= set(_lib.SIGNATURES)
    src = open(os.path.join(REPO, "include", "rvc_amd.h")).read()
    enum = dict(re.findall(r"(RVC_LFILTER_[A-Z_]+) = ([0-9* ]+)", src))
    assert {k: eval(v) for k, v in enum.items()} == {
        "RVC_LFILTER_CHUNK": _lib.LFILTER_CHUNK, "RVC_LFILTER_WAVE": _lib.LFILTER_WAVE,
        "RVC_LFILTER_TILE": _lib.LFILTER_TILE, "RVC_LFILTER_WARM_CAP": _lib.LFILTER_WARM_CAP}
    assert _lib.LFILTER_WAVE == 64 * _lib.LFILTER_CHUNK and _lib.LFILTER_CHUNK % _lib.LFILTER_TILE == 0


def test_entries_validate_before_any_launch():
    """Bad sizes and table rows are refused on the host (-22) with no device in the machine."""
    lib = _lib.load()
    b, a = signal.butter(N=5, Wn=48, btype="high", fs=32000)
    pb, pa = ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(a.ctypes.data)
    one = ctypes.c_void_p(8)  # non-null, never dereferenced
    assert lib.rvc_lfilter64(None, 0, 10, pb, pa, 8000, None, 0, one, None) == -22
    assert b"null" in lib.rvc_last_error()
    assert lib.rvc_lfilter64(one, 0, 0, pb, pa, 8000, None, 0, one, None) == -22
    assert lib.rvc_lfilter64(one, 0, 10, pb, pa, 8001, None, 0, one, None) == -22  # not a multiple of the tile
    assert lib.rvc_lfilter64(one, 0, 10, pb, pa, _lib.LFILTER_WARM_CAP + 32, None, 0, one, None) == -22
    assert b"warm-up" in lib.rvc_last_error()
    assert lib.rvc_lfilter64(one, 0, 1 << 31, pb, pa, 8000, None, 0, one, None) == -22
    assert lib.rvc_lfilter64_work_bytes(10, 8000) == 0 and lib.rvc_lfilter64_work_bytes(0, 8000) == -1
    assert lib.rvc_lfilter64_work_bytes(10, 8001) == -1
    assert lib.rvc_frame_rms64_len(153600, 1920, 480) == 321 and lib.rvc_frame_rms64_len(1, 1920, 480) == 1
    assert lib.rvc_frame_rms64_len(0, 1920, 480) == -1
    assert lib.rvc_frame_rms64(one, 1, 0, 1920, 480, one, None) == -22
    assert lib.rvc_frame_rms64(one, 1, 10, 0, 480, one, None) == -22
    assert lib.rvc_frame_rms64(one, 1, 10, 1920, -1, one, None) == -22
    assert lib.rvc_peak_mix64(one, 0, 0.675, 0.25, one, one, None) == -22
    assert lib.rvc_peak_mix64(one, 5, 0.675, 0.25, None, one, None) == -22

    def resample(seg, n_in=100, n_out=50, up=1, down=2, h_len=43, pre=10):
        seg = np.array(seg, np.int64).reshape(-1, 4)
        return lib.rvc_resample_poly64(one, 1, n_in, one, h_len, up, down, pre, ctypes.c_void_p(seg.ctypes.data),
                                       one, seg.shape[0], one, one, n_out, None)

    assert resample([0, 100, 0, 50], n_in=0) == -22
    assert resample([0, 100, 0, 50], up=0) == -22
    assert resample([1, 100, 0, 50]) == -22 and b"reads" in lib.rvc_last_error()  # input past the buffer
    assert resample([0, 100, 1, 50]) == -22 and b"writes" in lib.rvc_last_error()  # output past the buffer
    assert resample([0, 99, 0, 49]) == -22 and b"ceil" in lib.rvc_last_error()  # 99 / 2 rounds up to 50
    assert resample([0, 0, 0, 0]) == -22
    assert resample([-1, 10, 0, 5]) == -22
    assert resample([[0, 60, 0, 30], [40, 60, 30, 21]]) == -22  # the second row is checked too


def test_resample_plan_is_scipys():
    """The taps and bookkeeping handed to the kernel reproduce scipy.signal.resample_poly when applied directly."""
    rng = np.random.default_rng(5)
    for up, down in [(1, 2), (1, 3), (2, 5), (400, 441)]:
        h, n_pre_remove = pre.resample_taps(up, down)
        h2, r2 = R.resample_plan(up, down)
        assert np.array_equal(h, h2) and n_pre_remove == r2
        for n in (1, down, 997):
            x = rng.standard_normal(n)
            ref = signal.resample_poly(x, up, down)
            full = signal.upfirdn(h, x, up, down)
            m = -(-n * up // down)
            got = np.concatenate([full, np.zeros(max(n_pre_remove + m - full.size, 0))])[n_pre_remove: n_pre_remove + m]
            assert ref.shape == got.shape and np.abs(got - ref).max() <= R.resample_bound(up, down, np.abs(x).max())


def test_write_wav_f32_round_trip(tmp_path):
    x = (np.random.default_rng(0).standard_normal(1000) * 0.1)
    audio_io.write_wav_f32(str(tmp_path / "a.wav"), x, 32000)
    from scipy.io import wavfile
    sr, raw = wavfile.read(str(tmp_path / "a.wav"))
    assert sr == 32000 and raw.dtype == np.float32 and np.array_equal(raw, x.astype(np.float32))
    y, sr = audio_io.read_wav(str(tmp_path / "a.wav"))
    assert np.array_equal(y, raw)


def test_file_walk(tmp_path):
    for d in ("", "0", "1"):
        os.makedirs(tmp_path / d, exist_ok=True)
        (tmp_path / d / "b.wav").write_bytes(b"")
        (tmp_path / d / "a.WAV").write_bytes(b"")
        (tmp_path / d / "notes.txt").write_bytes(b"")
    files = pre.list_files(str(tmp_path))
    assert [(os.path.relpath(p, tmp_path), i, s) for p, i, s in files] == [
        ("a.WAV", 0, 0), ("b.wav", 1, 0), ("0/a.WAV", 2, 0), ("0/b.wav", 3, 0), ("1/a.WAV", 4, 1), ("1/b.wav", 5, 1)]
    os.makedirs(tmp_path / "x")
    with pytest.raises(ValueError, match="'x'"):
        pre.list_files(str(tmp_path))
