"""mangio-crepe-<capacity> f0 on the device (VC.get_f0_mangio_crepe, convert.py:215-228; FeatureInput.get_mangio_crepe,
extract.py:162-171) against the reference's recorded output (tests/golden/mangio.npz, make_golden_mangio.py) and the
numpy restatement of everything behind the network (tests/mangio_ref.py).  crepe-tiny only."""
import numpy as np
import pytest
import torch

import mangio_ref
from rvc_amd import f0mix, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOPS = (37, 64, 160, 512)
P_LEN = 75
RTOL, ATOL = 1e-4, 1e-3  # tests/test_gpu_crepe.py's bounds for the same arithmetic


@pytest.fixture(scope="module")
def setup(golden):
    from rvc_amd.crepe import CrepeAMD
    from rvc_amd.extract import FeatureInputAMD
    from rvc_amd.pipeline import VC, Config
    g = golden("mangio")
    m = CrepeAMD(synthetic.crepe_state_dict(int(g["seeds"][0]), "tiny"), "tiny", DEV)
    by_T = {len(g[f"dither_{h}"]): g[f"dither_{h}"] for h in HOPS}  # one frame count per hop
    m.dither_fn = lambda T: by_T[T]
    cfg = Config(DEV)
    cfg.x_pad = 0  # the f0 file starts at frame 0, as in the golden
    vc = VC(40000, cfg, crepe={"tiny": m})
    fi = FeatureInputAMD(device=DEV, crepe={"tiny": m})
    return g, m, vc, fi, torch.from_numpy(g["x"]).to(DEV)


# ------------------------------------------------------------------ rvc_f0_resample_nan
def _sources(T, rng):
    """Random tracks in 40..900 Hz with values below 0.001 first / last / alone between equal neighbours / as an
    adjacent pair, and two with an infinite value (np.interp's two NaN fallbacks)."""
    base = rng.uniform(40, 900, T).astype(np.float32)
    low = np.float32(0.0005)
    out = []
    for where in ("first", "last", "alone", "pair", "inf", "infs"):
        s = base.copy()
        mid = T // 2
        if where == "first":
            s[0] = low
        elif where == "last":
            s[-1] = 0
        elif where == "alone":
            s[mid] = low
            if 0 < mid < T - 1:
                s[mid + 1] = s[mid - 1]  # equal neighbours around the gap
        elif where == "pair":
            s[mid: mid + 2] = 0
        elif where == "inf":
            s[mid] = np.inf
        else:
            s[mid: mid + 2] = np.inf
        out.append((where, s))
    return out


@pytest.mark.parametrize("p_len", [1, 2, 75, 76, 300])
@pytest.mark.parametrize("T", [1, 2, 24, 76, 189])
def test_resample_matches_numpy_bit_for_bit(T, p_len):
    rng = np.random.default_rng(1000 * T + p_len)
    for where, src in _sources(T, rng):
        source = src.copy()
        with np.errstate(invalid="ignore"):
            source[source < 0.001] = np.nan
            want = np.nan_to_num(np.interp(np.arange(0, len(source) * p_len, len(source)) / p_len,
                                           np.arange(0, len(source)), source))
        got = ops.f0_resample_nan(torch.from_numpy(src).to(DEV), p_len).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (p_len,)
        assert got.tobytes() == want.tobytes(), (where, np.flatnonzero(got != want)[:5], got[:4], want[:4])


# ------------------------------------------------------------------ decode of the reference's probabilities
def _ulps(a, b):
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32))


def _bins(f0_raw, dither):
    """The Viterbi bin behind each raw f0: 20 cents a bin against an f32 error of a fraction of a cent."""
    cents = 1200 * np.log2(f0_raw.astype(np.float64) / 10) - 1997.3794084376191 - dither[: len(f0_raw)]
    b = np.rint(cents / 20)
    assert np.abs(cents / 20 - b).max() < 0.01
    return b.astype(np.int64)


@pytest.mark.parametrize("hop", HOPS)
def test_decode_of_reference_probabilities(setup, hop):
    g, m, _, _, _ = setup
    probs = torch.from_numpy(np.ascontiguousarray(g[f"probs_{hop}"].T)).to(DEV)  # [360][T]
    tr = {}
    f0 = m.decode_mangio(probs, hop, P_LEN, trace=tr).cpu().numpy()
    np.testing.assert_array_equal(_bins(tr["f0_raw"], g[f"dither_{hop}"]), g[f"bins_{hop}"])
    assert f0.dtype == np.float64
    np.testing.assert_allclose(f0, g[f"f0_{hop}"], rtol=RTOL, atol=ATOL)


def test_decode_without_restart_would_differ(setup):
    """The 2 * hop segments are what the decode above is about: one segment gives other bins."""
    g, m, _, _, _ = setup
    probs = torch.from_numpy(np.ascontiguousarray(g["probs_64"].T)).to(DEV)
    tr = {}
    m.decode_mangio(probs, 512, P_LEN, trace=tr)  # 2 * 512 >= T: one segment
    assert (_bins(tr["f0_raw"], g["dither_64"]) != g["bins_64"]).sum() >= 100


def test_bins_to_hz_is_the_vector_path(setup):
    """rvc_crepe_decode_as(RVC_CREPE_HZ_TORCH): every admissible bin under random dither, one-frame segments (the
    Viterbi is then the argmax), against mangio_ref.pow2_vector -- the vector path of torch's CPU pow restated in
    NumPy, so the expected values depend on neither the host nor the tensor's length (tests/test_mangio_cpu.py holds
    that restatement to torch itself) -- in every bit; the powf form of rvc_crepe_decode stays within 2 ulp of it and
    is not the same function."""
    from rvc_amd import crepe
    g, m, _, _, _ = setup
    rng = np.random.default_rng(5)
    bins = np.concatenate([np.arange(m.lo, m.hi), rng.integers(m.lo, m.hi, 4000)]).astype(np.int64)
    T = len(bins)
    dither = rng.triangular(-20, 0, 20, size=T)
    probs = np.full((360, T), 0.01, np.float32)
    probs[bins, np.arange(T)] = 0.9
    dd = torch.from_numpy(dither.astype(np.float32)).to(DEV)
    want = mangio_ref.bins_to_hz(bins, dither, vector=True)
    got = {}
    for hz in (crepe.HZ_TORCH, crepe.HZ_POWF):
        f0r, pd = m._decode(torch.from_numpy(probs).to(DEV), list(range(T + 1)), dd, hz)
        got[hz] = f0r.cpu().numpy()
        assert (pd.cpu().numpy() == np.float32(0.9)).all()  # the chosen bin is the planted one
    assert want.dtype == np.float32 and got[crepe.HZ_TORCH].tobytes() == want.tobytes()
    assert _ulps(got[crepe.HZ_POWF], want).max() <= 2 and not np.array_equal(got[crepe.HZ_POWF], want)


# ------------------------------------------------------------------ network: framing at the hop, the normalisation
@pytest.mark.parametrize("hop", [37, 64])
def test_network_matches_reference(setup, hop):
    g, m, _, _, x = setup
    tr = {}
    m.f0_mangio(f0mix.normalize(x), hop, P_LEN, trace=tr)
    assert tr["probs"].shape == g[f"probs_{hop}"].shape
    err = np.abs(tr["probs"] - g[f"probs_{hop}"]).max()
    print(f"hop {hop}: max |probs - reference| = {err:.3g}")
    assert err < 2e-5, err


def test_hybrid_member_is_normalised_twice(setup):
    """Inside a hybrid the signal get_f0_hybrid divided is divided again by get_f0_mangio_crepe."""
    g, m, vc, _, x = setup
    xn = f0mix.normalize(x)
    once = vc.f0_raw(x, "mangio-crepe-tiny", P_LEN, 64)
    twice = vc.f0_raw(xn, "mangio-crepe-tiny", P_LEN, 64)
    want = m.f0_mangio(f0mix.normalize(xn), 64, P_LEN)
    assert torch.equal(twice, want) and torch.equal(once, m.f0_mangio(xn, 64, P_LEN))
    np.testing.assert_allclose(once.cpu().numpy(), g["f0_64"], rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ end to end
def _device_run(m, xn, hop):
    """The device's own probabilities [T][360] and raw f32 track [T] for the normalised signal xn."""
    tr = {}
    m.f0_mangio(xn, hop, P_LEN, trace=tr)
    return tr["probs"], tr["f0_raw"]


def _check_reference(name, c, f, ref_c, ref_f):
    """The decode bounds against the reference; coarse equal in >= 99 % of the frames and never off by more than 1."""
    assert c.shape == ref_c.shape and f.shape == ref_f.shape
    print(f"{name}: max |f0 - reference| {np.abs(f - ref_f).max():.3g} Hz, coarse equal {np.mean(c == ref_c):.3f}")
    np.testing.assert_allclose(f, ref_f, rtol=RTOL, atol=ATOL)
    assert np.mean(c == ref_c) >= 0.99 and np.abs(c - ref_c).max() <= 1


@pytest.mark.parametrize("variant", ["plain", "tune", "file"])
def test_get_f0_matches_reference(setup, variant):
    """VC.f0_device against the reference's get_f0; and, exactly: the bins are the restated Viterbi's on the device's
    own probabilities, and (coarse, pitchf) are the restated f64 tail (resample, autotune, shift, f0 file, quantiser) of the
    device's own f32 track."""
    g, m, vc, _, x = setup
    pitch, autotune, strength, f0_file = mangio_ref.variants()[variant]
    coarse, pitchf = vc.f0_device(x, pitch, "mangio-crepe-tiny", autotune, strength, f0_file, hop_length=64)
    c, f = coarse.cpu().numpy(), pitchf.cpu().numpy()
    assert f.dtype == np.float32
    _check_reference(variant, c, f, g[f"vc:{variant}:coarse"], g[f"vc:{variant}:pitchf"])
    probs, f0_raw = _device_run(m, f0mix.normalize(x), 64)
    np.testing.assert_array_equal(_bins(f0_raw, g["dither_64"]),
                                  mangio_ref.viterbi_bins(probs, mangio_ref.segments(len(probs), 64)))
    own_c, own_f = mangio_ref.get_f0(mangio_ref.resample(f0_raw, P_LEN), pitch, strength if autotune else None, f0_file)
    assert f.tobytes() == own_f.astype(np.float32).tobytes()
    np.testing.assert_array_equal(c, own_c)


def test_extraction_matches_reference(setup):
    g, m, _, fi, x = setup
    f0 = fi.compute_f0(g["x"], "mangio-crepe-tiny", 64)
    assert f0.dtype == np.float64
    _check_reference("extract", fi.coarse_f0(f0), f0, fi.coarse_f0(g["fi_f0"]), g["fi_f0"])
    # get_mangio_crepe divides by torch.quantile, get_f0_mangio_crepe by np.quantile: each scale to the bit
    assert np.float32(float(f0mix.abs_quantile(x, f0mix.QUANTILE_TORCH))).tobytes() == \
        mangio_ref.scale_extract(g["x"]).tobytes()
    assert np.float32(float(f0mix.abs_quantile(x))).tobytes() == mangio_ref.scale_convert(g["x"]).tobytes()
    probs, f0_raw = _device_run(m, f0mix.normalize(x, f0mix.QUANTILE_TORCH), 64)
    assert f0.tobytes() == mangio_ref.resample(f0_raw, P_LEN).tobytes()
    # inside hybrid[...] the extraction path does not pre-normalise: one member is the method alone, resampled
    hy = fi.compute_f0(g["x"], "hybrid[mangio-crepe-tiny]", 64)
    np.testing.assert_array_equal(hy, np.interp(np.linspace(0, len(f0), P_LEN), np.arange(len(f0)), f0))


@pytest.mark.parametrize("route", ["plain", "tune", "file", "extract"])
def test_bit_equal_to_restatement_on_own_probabilities(setup, route):
    """The whole of mangio_ref -- Viterbi per batch, bins -> Hz, resample, get_f0's tail -- on the device's own
    probabilities, against the device, bit for bit.

    bins -> Hz is the one f32 transcendental of the chain.  The restatement takes it in the form that depends on no
    host (``vector=True``: the vector path of torch's CPU pow for every frame), which is what the device computes.  The
    reference itself computes the tail frames of each batch (61 = 32 + 29 at this hop on a 16-lane host) with the C
    library's powf; tests/test_mangio_cpu.py pins that the golden's hop-64 track is the same in both forms."""
    g, m, vc, fi, x = setup
    if route == "extract":
        probs, f0_raw = _device_run(m, f0mix.normalize(x, f0mix.QUANTILE_TORCH), 64)
        got = fi.compute_f0(g["x"], "mangio-crepe-tiny", 64)
        want = mangio_ref.f0(probs, 64, g["dither_64"], P_LEN, vector=True)
    else:
        pitch, autotune, strength, f0_file = mangio_ref.variants()[route]
        probs, f0_raw = _device_run(m, f0mix.normalize(x), 64)
        got = vc.f0_device(x, pitch, "mangio-crepe-tiny", autotune, strength, f0_file, hop_length=64)[1].cpu().numpy()
        want = mangio_ref.get_f0(mangio_ref.f0(probs, 64, g["dither_64"], P_LEN, vector=True), pitch,
                                 strength if autotune else None, f0_file)[1].astype(np.float32)
    source = mangio_ref.postprocess(probs, 64, g["dither_64"], vector=True)[1]
    print(f"{route}: f0 bits equal in {np.mean(got == want):.3f} of the frames, max |difference| "
          f"{np.abs(got - want).max():.3g} Hz; f32 track: {np.mean(f0_raw == source):.3f} equal, at most "
          f"{_ulps(f0_raw, source).max()} ulp apart")
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ ClipGraph
@pytest.fixture(scope="module")
def models():
    from rvc_amd.crepe import CrepeAMD
    from test_gpu_graph import build
    vc, hub, net_g = build()
    vc.crepe["tiny"] = CrepeAMD(synthetic.crepe_state_dict(1241, "tiny"), "tiny", DEV)
    a = torch.from_numpy(synthetic.synthetic_audio(2.0, seed=1003)).to(DEV)  # longer than the 1 s reflect padding
    return vc, hub, net_g, a


def test_clip_graph_forwards_hop_length(models):
    """Replays equal the eager pass at the same device seed and hop; another hop gives another waveform (the
    pattern of tests/test_gpu_graph.py)."""
    from rvc_amd.graph import ClipGraph
    vc, hub, net_g, a = models
    method = "mangio-crepe-tiny"

    def eager(seed, hop):
        t = torch.full((1,), seed, dtype=torch.int64, device=DEV)  # graph-mode draws (device dither) at 0 + seed
        vc.seed = 0
        with ops.device_seed(t):
            return vc.pipeline_device(hub, net_g, 0, a, 0, "v2", 0.33, None, 0.0, method, hop_length=hop).clone()

    g37 = ClipGraph(vc, hub, net_g, 0, a.numel(), f0_method=method, hop_length=37)
    got = g37(a, 9).clone()
    again = g37(a, 9).clone()
    torch.cuda.synchronize()
    ref = eager(9, 37)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(again, ref)
    g64 = ClipGraph(vc, hub, net_g, 0, a.numel(), f0_method=method, hop_length=64)
    other = g64(a, 9).clone()
    torch.cuda.synchronize()
    assert torch.equal(other, eager(9, 64))
    assert not torch.equal(other, got)
    assert np.isfinite(got.cpu().numpy()).all()


def test_batch_and_stream_forward_hop_length(models):
    """pipeline_device_batch and pipeline_device_stream hand ``hop_length`` to the f0 method: at hop 37 each gives the
    per-call pass at hop 37 (the stream bit for bit at batch 1, the batch up to its batched launches' summation order)
    and not the waveform of hop 64."""
    vc, hub, net_g, a = models
    method = "mangio-crepe-tiny"
    dither = np.random.default_rng(7).triangular(-20, 0, 20, size=4000)
    vc.crepe["tiny"].dither_fn = lambda T: dither[:T]
    try:
        vc.seed = 40
        args = (hub, net_g, 0, [a, a], 0, "v2", 0.33)
        b37 = vc.pipeline_device_batch(*args, f0_method=method, hop_length=37)
        b64 = vc.pipeline_device_batch(*args, f0_method=method, hop_length=64)
        s37 = vc.pipeline_device_stream(*args, f0_method=method, hop_length=37)
        s64 = vc.pipeline_device_stream(*args, f0_method=method, hop_length=64)
        for k in range(2):
            vc.seed = 40 + k
            ref = vc.pipeline_device(hub, net_g, 0, a, 0, "v2", 0.33, None, 0.0, method, hop_length=37)
            assert torch.equal(s37[k], ref), float((s37[k] - ref).abs().max())
            rel = ((b37[k] - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()
            assert rel <= 1e-4, (k, rel)
            assert not torch.equal(s64[k], s37[k]) and not torch.equal(b64[k], b37[k])
    finally:
        vc.crepe["tiny"].dither_fn = None
        vc.seed = 0
