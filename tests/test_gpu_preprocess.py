"""Dataset preprocessing on the device (csrc/preprocess.hip, rvc_amd/preprocess.py): each kernel against scipy /
numpy at the sizes where its code changes path, the whole chain against the reference's own output
(tests/golden/preprocess*.npz), and the wiring of preprocess_training_set."""
import os

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

import preprocess_ref as R
from rvc_amd import _lib, audio_io, edges, synthetic
from rvc_amd import preprocess as pre

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUT = [(0.3, 0), (2.0, 1), (0.6, 0), (1.7, 1), (0.2, 0)]
CHUNK, WAVE = _lib.LFILTER_CHUNK, _lib.LFILTER_WAVE
U = 2.0 ** -53


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---------------------------------------------------------------- lfilter
LF_N = 400000


@pytest.fixture(scope="module")
def lf_cases():
    """Per rate: the filter, its warm-up, the input (DC + 30 Hz + noise: what a short warm-up leaks) and scipy's
    two forms of the output over the longest length.  The filter is causal, so every shorter case is a prefix."""
    out = {}
    for sr in (16000, 48000):
        b, a = signal.butter(N=5, Wn=48, btype="high", fs=sr)
        sos = signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos")
        rng = np.random.default_rng(sr)
        t = np.arange(LF_N) / sr
        x = (0.3 + 0.4 * np.sin(2 * np.pi * 30 * t) + 0.1 * rng.standard_normal(LF_N)).astype(np.float32)
        out[sr] = dict(b=b, a=a, warm=pre.warmup(b, a), x=x, ref=signal.lfilter(b, a, x),
                       sos=signal.sosfilt(sos, x.astype(np.float64)))
    return out


def lf_lengths(warm):
    return [1, 5, 6, CHUNK - 1, CHUNK, CHUNK + 1, WAVE + 1, warm + CHUNK + 1, LF_N]


@pytest.mark.parametrize("which", range(9))
@pytest.mark.parametrize("sr", [16000, 48000])
def test_lfilter_matches_scipy(lf_cases, sr, which):
    c = lf_cases[sr]
    n = lf_lengths(c["warm"])[which]
    x, ref = c["x"][:n], c["ref"][:n]
    if n in (1, 6, CHUNK + 1):  # the prefix property the shared reference leans on
        assert np.array_equal(signal.lfilter(c["b"], c["a"], x), ref)
    e = np.abs(ref - c["sos"][:n]).max()
    y = pre.lfilter(dev(x), c["b"], c["a"], c["warm"])
    assert y.dtype == torch.float64 and y.shape == (n,)
    y = y.cpu().numpy()
    err = np.abs(y - ref).max()
    print(f"lfilter sr={sr} N={n} warm={c['warm']}: err {err:.3g}, e {e:.3g}, tol {max(2 * e, 1e-12):.3g}")
    assert not np.isnan(y).any() and err <= max(2 * e, 1e-12)
    again = pre.lfilter(dev(x), c["b"], c["a"], c["warm"]).cpu().numpy()
    assert np.array_equal(again, y)
    from64 = pre.lfilter(dev(x.astype(np.float64)), c["b"], c["a"], c["warm"]).cpu().numpy()
    assert np.array_equal(from64, y)


def test_lfilter_rejects_bad_input():
    b, a = signal.butter(N=5, Wn=48, btype="high", fs=32000)
    with pytest.raises(TypeError):
        pre.lfilter(torch.zeros(10), b, a)  # host tensor
    with pytest.raises(RuntimeError, match="warm-up"):
        pre.lfilter(torch.zeros(10, device=DEV), b, a, warm=100)


# ---------------------------------------------------------------- frame RMS
@pytest.mark.parametrize("n,frame,hop", [(1, 1920, 480), (479, 1920, 480), (480, 1920, 480), (1920, 1920, 480),
                                         (153600, 1920, 480), (100001, 2880, 720)])
def test_frame_rms_matches_get_rms(n, frame, hop):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * np.exp(rng.uniform(-9, 0, n))  # levels from -80 dB to full scale
    ref = edges.get_rms(x, frame, hop).squeeze(0)
    out = pre.frame_rms(dev(x), frame, hop)
    assert out.dtype == torch.float64 and tuple(out.shape) == ref.shape == (1 + n // hop,)
    out = out.cpu().numpy()
    rel = np.abs(out - ref) / ref
    print(f"rms n={n}: rel err {rel.max():.3g}, bound {(frame + 8) * U:.3g}")
    assert (ref > 0).all() and rel.max() <= (frame + 8) * U
    assert np.array_equal(pre.frame_rms(dev(x), frame, hop).cpu().numpy(), out)
    x32 = x.astype(np.float32)  # f32 samples: the same f64 sums over the same values
    assert np.array_equal(pre.frame_rms(dev(x32), frame, hop).cpu().numpy(),
                          pre.frame_rms(dev(x32.astype(np.float64)), frame, hop).cpu().numpy())


# ---------------------------------------------------------------- peak mix
@pytest.mark.parametrize("where", ["first", "last", "negative"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_peak_mix_is_numpys_bits(n, where):
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.9, 0.9, n)
    x[{"first": 0, "last": n - 1, "negative": n // 2}[where]] = -1.7 if where == "negative" else 1.7
    peak = np.abs(x).max()
    ref = (x / peak * (pre.MAX_AMPLITUDE * pre.ALPHA)) + (1 - pre.ALPHA) * x
    y, cell = pre.peak_mix(dev(x))
    assert float(cell.item()) == peak == 1.7
    assert np.array_equal(y.cpu().numpy(), ref)


def test_peak_above_the_limit_is_reported():
    x = np.random.default_rng(0).uniform(-1, 1, 1000)
    x[777] = -2.6
    _, cell = pre.peak_mix(dev(x))
    assert float(cell.item()) == 2.6 > 2.5


# ---------------------------------------------------------------- resample
RATIOS = [(1, 2), (1, 3), (2, 5), (400, 441)]


def span(up, down):
    return -(-R.resample_plan(up, down)[0].size // up)  # input samples under the filter


@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_matches_scipy(up, down):
    rng = np.random.default_rng(up * 1000 + down)
    for n in sorted({1, 2, down - 1, down, span(up, down) + 1, 25280}):
        x = rng.uniform(-1, 1, n)
        ref = signal.resample_poly(x, up, down)
        y64, y32, spans = pre.resample_poly(dev(x), up, down)
        assert spans == [(0, ref.size)] and y64.dtype == torch.float64 and y32.dtype == torch.float32
        y64, y32 = y64.cpu().numpy(), y32.cpu().numpy()
        err, bound = np.abs(y64 - ref).max(), R.resample_bound(up, down, np.abs(x).max())
        print(f"resample {up}/{down} n={n}: err {err:.3g}, bound {bound:.3g}")
        assert y64.shape == ref.shape and err <= bound
        assert np.array_equal(y32, y64.astype(np.float32))


@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_chunks_are_independent(up, down):
    """Three unequal chunks in one launch: the bits of three launches, whatever lies next to them."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, 6000)
    chunks = [(100, 1300), (1400, 257), (1500, 3001)]  # touching, and overlapping as preprocess's chunks do
    y64, y32, spans = pre.resample_poly(dev(x), up, down, chunks)
    y64, y32 = y64.cpu().numpy(), y32.cpu().numpy()
    assert [m for _, m in spans] == [-(-n * up // down) for _, n in chunks] and spans[0][0] == 0
    for (o, n), (p, m) in zip(chunks, spans):
        alone, alone32, _ = pre.resample_poly(dev(x[o: o + n].copy()), up, down)
        assert np.array_equal(y64[p: p + m], alone.cpu().numpy())
        assert np.array_equal(y32[p: p + m], alone32.cpu().numpy())
    other = x.copy()
    other[:100] = 9.0  # everything outside the first chunk changes
    other[1400:] = -9.0
    z64, _, _ = pre.resample_poly(dev(other), up, down, chunks)
    p, m = spans[0]
    assert np.array_equal(z64.cpu().numpy()[p: p + m], y64[p: p + m])
    assert not np.array_equal(z64.cpu().numpy()[spans[2][0]:], y64[spans[2][0]:])


def test_resample_rejects_a_chunk_past_the_buffer():
    with pytest.raises(RuntimeError, match="reads"):
        pre.resample_poly(torch.zeros(100, dtype=torch.float64, device=DEV), 1, 2, [(50, 51)])


# ---------------------------------------------------------------- the chain against the reference's output
@pytest.fixture(scope="module")
def fixture_run(tmp_path_factory):
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess.npz")))
    for part in ("preprocess_gt_a", "preprocess_gt_b", "preprocess_16k"):
        g.update(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", part + ".npz")))
    sr, per, seed = int(g["args"][0]), float(g["args"][1]), int(g["args"][2])
    root = tmp_path_factory.mktemp("pre_model")
    wav = str(root / "input.wav")
    audio_io.write_wav_f32(wav, synthetic.silence_layout_audio(LAYOUT, seed=seed, sr=sr), sr)
    pp = pre.PreProcessAMD(sr, str(root / "exp"), per, DEV)
    out = pp.process_audio(wav, 0, 0, True, True, False, 0.7)
    return g, pp, out


def test_model_plan_matches_reference(fixture_run):
    g, pp, out = fixture_run
    assert out["names"] == list(g["names"])
    assert np.array_equal(out["offsets"], g["offsets"])
    assert sorted(os.listdir(pp.gt_wavs_dir)) == sorted(os.listdir(pp.wavs16k_dir)) == sorted(g["names"])
    peak = max(np.abs(g[f"gt_{k}"]).max() for k in range(len(g["names"])))
    filt = float(g["tol_gt"]) - 2.0 ** -24 * float(peak)  # the filter's share of tol_gt; RMS moves by at most that
    assert filt > 0 and out["rms"].shape == g["rms"].shape
    bound = (pp.slicer.win_size + 8) * U * g["rms"] + filt
    print("rms err", np.abs(out["rms"] - g["rms"]).max(), "bound", bound.min())
    assert (np.abs(out["rms"] - g["rms"]) <= bound).all()


def test_model_slices_match_reference(fixture_run):
    g, pp, out = fixture_run
    for k, name in enumerate(out["names"]):
        for folder, sr, key, tol in ((pp.gt_wavs_dir, pp.sr, f"gt_{k}", g["tol_gt"]),
                                     (pp.wavs16k_dir, 16000, f"k16_{k}", g["tol_16k"])):
            rate, raw = wavfile.read(os.path.join(folder, name))
            assert rate == sr and raw.dtype == np.float32  # an IEEE-float WAV
            x, rate = audio_io.read_wav(os.path.join(folder, name))
            assert rate == sr and np.array_equal(x, raw)
            assert x.shape == g[key].shape == (g["lengths"][k][0 if sr == pp.sr else 1],)
            err = np.abs(x.astype(np.float64) - g[key]).max()
            print(f"{name} @{sr}: err {err:.3g}, tol {float(tol):.3g}")
            assert err <= tol


# ---------------------------------------------------------------- wiring
def tree_bytes(d):
    return {os.path.join(sub, f): open(os.path.join(d, sub, f), "rb").read()
            for sub in ("sliced_audios", "sliced_audios_16k") for f in sorted(os.listdir(os.path.join(d, sub)))}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("pre_data")
    sr = 32000
    layouts = {"root.wav": [(0.2, 0), (1.6, 1), (0.6, 0), (1.0, 1)], "0/a.wav": [(1.7, 1)],
               "1/b.wav": [(0.1, 0), (2.2, 1), (0.1, 0)]}
    for k, (rel, layout) in enumerate(layouts.items()):
        os.makedirs(os.path.dirname(root / "in" / rel), exist_ok=True)
        audio_io.write_wav_f32(str(root / "in" / rel), synthetic.silence_layout_audio(layout, seed=6200 + k, sr=sr), sr)
    (root / "in" / "readme.txt").write_text("not audio")
    return root, sr


def test_ranks_write_what_one_process_writes(dataset):
    root, sr = dataset
    one = pre.preprocess_training_set(str(root / "in"), sr, 4, str(root / "w1"), 1.0, True, True, False, 0.7, DEV)
    r0 = pre.preprocess_training_set(str(root / "in"), sr, 4, str(root / "w2"), 1.0, True, True, False, 0.7, DEV,
                                     rank=0, world=2)
    r1 = pre.preprocess_training_set(str(root / "in"), sr, 4, str(root / "w2"), 1.0, True, True, False, 0.7, DEV,
                                     rank=1, world=2)
    assert sorted(one) == sorted(r0 + r1) and not set(r0) & set(r1) and r0 and r1
    # idx0 numbers every file before sharding; sid is the folder's name (0 for the root)
    assert {tuple(n.split("_")[:2]) for n in one} == {("0", "0"), ("0", "1"), ("1", "2")}
    a, b = tree_bytes(str(root / "w1")), tree_bytes(str(root / "w2"))
    assert a.keys() == b.keys() and len(a) == 2 * len(one) and all(a[k] == b[k] for k in a)


def test_non_integer_folder_raises(dataset, tmp_path):
    root, sr = dataset
    os.makedirs(tmp_path / "in" / "x")
    with pytest.raises(ValueError, match="'x'"):
        pre.preprocess_training_set(str(tmp_path / "in"), sr, 1, str(tmp_path / "exp"), 1.0, True, True, False, 0.7,
                                    DEV)


def test_options(dataset):
    root, sr = dataset
    names = pre.preprocess_training_set(str(root / "in"), sr, 1, str(root / "nocut"), 1.0, False, False, False, 0.7,
                                        DEV)
    assert sorted(names) == ["0_0_0.wav", "0_1_0.wav", "1_2_0.wav"]  # one slice per file
    for name, rel in (("0_0_0.wav", "root.wav"), ("0_1_0.wav", "0/a.wav"), ("1_2_0.wav", "1/b.wav")):
        loaded = audio_io.load_audio(str(root / "in" / rel), sr)
        x, rate = audio_io.read_wav(str(root / "nocut" / "sliced_audios" / name))
        assert rate == sr and np.array_equal(x, loaded)  # no effects: the slice is the input, bit for bit
        y, rate = audio_io.read_wav(str(root / "nocut" / "sliced_audios_16k" / name))
        assert rate == 16000 and y.shape == (-(-loaded.size // 2),)
        assert np.abs(y - signal.resample_poly(loaded.astype(np.float64), 1, 2)).max() <= \
            R.resample_bound(1, 2, np.abs(loaded).max()) + 2.0 ** -24 * np.abs(y).max()
    # effects without cutting: one slice, the filtered and mixed whole file
    pp = pre.PreProcessAMD(sr, str(root / "fx"), 1.0, DEV)
    out = pp.process_audio(str(root / "in" / "0" / "a.wav"), 5, 3, False, True, False, 0.7)
    assert out["names"] == ["3_5_0.wav"] and out["rms"] is None
    loaded = audio_io.load_audio(str(root / "in" / "0" / "a.wav"), sr)
    want = R.chain(loaded, sr, 1.0, cut_preprocess=False)["gt"][0].astype(np.float64)
    sos = R.chain(loaded, sr, 1.0, cut_preprocess=False, filt="sosfilt")["gt"][0]
    tol = 2 * np.abs(want - sos).max() + 2.0 ** -24 * np.abs(want).max()  # the fixture's yardstick on this input
    x, _ = audio_io.read_wav(os.path.join(pp.gt_wavs_dir, "3_5_0.wav"))
    assert x.shape == want.shape and np.abs(x - want).max() <= tol


def test_peak_over_limit_follows_the_reference(tmp_path):
    sr = 32000
    x = synthetic.silence_layout_audio([(1.2, 1)], seed=3, sr=sr) * np.float32(40.0)
    wav = str(tmp_path / "loud.wav")
    audio_io.write_wav_f32(wav, x, sr)
    pp = pre.PreProcessAMD(sr, str(tmp_path / "exp"), 1.0, DEV)
    with pytest.raises(RuntimeError):
        pp.process_audio(wav, 0, 0, True, True, False, 0.7)  # the slicer would have received None
    out = pp.process_audio(wav, 0, 0, False, True, False, 0.7)  # only process_audio_segment would: skipped
    assert out["names"] == [] and os.listdir(pp.gt_wavs_dir) == []


def test_clean_dataset_runs_the_gate(dataset):
    """clean_dataset: the existing spectral gate between the mix and the slicer, on the device tensor as it is;
    the slicer and the resampler then take the gate's f32 samples."""
    from rvc_amd import denoise
    root, sr = dataset
    path = str(root / "in" / "1" / "b.wav")
    pp = pre.PreProcessAMD(sr, str(root / "clean"), 1.0, DEV)
    out = pp.process_audio(path, 2, 1, True, True, True, 0.7)
    y, _ = pre.peak_mix(pre.lfilter(dev(audio_io.load_audio(path, sr)), pp.b_high, pp.a_high, pp.warm))
    gated = denoise.reduce_noise(y=y, sr=sr, prop_decrease=0.7, device=DEV)
    assert gated.dtype == torch.float32
    want = gated.cpu().numpy()
    assert not np.array_equal(want, y.cpu().numpy().astype(np.float32))  # the gate changed the signal
    assert len(out["names"]) >= 2 and out["names"][0] == "1_2_0.wav"
    for name, (o, n) in zip(out["names"], out["offsets"]):
        x, _ = audio_io.read_wav(os.path.join(pp.gt_wavs_dir, name))
        assert np.array_equal(x, want[o: o + n])
        k16, _ = audio_io.read_wav(os.path.join(pp.wavs16k_dir, name))
        ref = signal.resample_poly(want[o: o + n].astype(np.float64), 1, 2)
        assert np.abs(k16 - ref).max() <= R.resample_bound(1, 2, np.abs(want).max()) + 2.0 ** -24 * np.abs(ref).max()
