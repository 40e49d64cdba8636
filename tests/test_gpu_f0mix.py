"""hybrid[a+b+...] f0 on the device (csrc/f0mix.hip, rvc_amd/f0mix.py): the 0.999 |x| quantile and the division by
it against NumPy bit for bit, the resample-and-median mix against np.interp / np.nanmedian, and the two hybrid
forms (VC.f0_device: normalised input, p_len frames; FeatureInputAMD.compute_f0: raw input, N // 160 frames)
against the mix of their members' own raw tracks."""
import numpy as np
import pytest
import torch

from rvc_amd import f0mix, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _signal(n, kind):
    rng = np.random.default_rng(n)
    if kind == "speech":
        return synthetic.synthetic_audio(n / 16000 + 0.01, seed=n % 97)[:n].astype(np.float32)
    if kind == "steps":  # many equal values: the two order statistics fall inside runs of equal samples
        return (np.round(rng.standard_normal(n) * 4) / 4).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", [1001, 2000, 16037, 160000])
@pytest.mark.parametrize("kind", ["noise", "steps", "speech"])
def test_abs_quantile_and_division_bit_identical_to_numpy(n, kind):
    x = _signal(n, kind)
    assert x.shape == (n,)
    want = np.quantile(np.abs(x), 0.999)
    assert want.dtype == np.float32
    xd = torch.from_numpy(x).to(DEV)
    got = f0mix.abs_quantile(xd).cpu().numpy()[0]
    assert got.tobytes() == want.tobytes(), (got, want)
    np.testing.assert_array_equal(f0mix.normalize(xd).cpu().numpy(), x / want)


def _tracks(p_len):
    rng = np.random.default_rng(p_len)

    def f0(n, dtype):
        v = 100 + 300 * rng.random(n)
        v[rng.random(n) < 0.3] = 0.0  # unvoiced frames
        return v.astype(dtype)

    a = f0(p_len + 1, np.float64)            # rmvpe-like: one frame more than p_len
    b = f0(p_len, np.float64)                # pm-like: padded to p_len
    c = f0(p_len + 1, np.float32)            # crepe / swipe-like
    d = f0(p_len // 2 + 3, np.float32)       # another hop
    b[5], c[p_len // 2], d[1] = np.nan, np.nan, np.nan
    a[7] = b[7] = c[7] = d[3] = 0.0
    return [a, b, c, d]


def _mix_numpy(tracks, p_len):
    rs = [np.interp(np.linspace(0, len(t), p_len), np.arange(len(t)), t) for t in tracks]
    return rs[0] if len(rs) == 1 else np.nanmedian(np.vstack(rs), axis=0)


def _post_f64(f0, pitch, autotune_strength=None):
    from oracle import pipeline as opl
    return opl.coarse_f0(np.array(f0), pitch, opl.Consts(40000), autotune_strength)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("p_len", [301, 1000])
def test_mix_matches_numpy(M, p_len):
    """np.interp over np.linspace, then np.nanmedian (mean of the middle two for an even count, NaNs ignored):
    the f64 mix equal to <= 1 ulp, then coarse and pitchf of the f64 post exact on the device's own mix."""
    import warnings
    from rvc_amd import _lib, ops, pm
    tracks = _tracks(p_len)[:M]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN slices
        want = _mix_numpy(tracks, p_len)
    dev = [torch.from_numpy(t).to(DEV) for t in tracks]
    mixed = f0mix.mix(dev, p_len)
    got = mixed.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (p_len,)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok])))
    mixed = torch.nan_to_num(mixed)  # (the quantiser's NaN handling is not what this test is about)
    coarse = torch.empty(p_len, dtype=torch.int64, device=DEV)
    pitchf = torch.empty(p_len, device=DEV)
    post = ops.F0Post(0.7, None, 0, DEV)
    ops.check(_lib.load().rvc_pm_post(pm._p64(mixed), p_len, p_len, float(2.0 ** (-2 / 12)), ops._post_ref(post, p_len),
                                      ops._p(coarse), ops._p(pitchf), ops._stream()), "pm_post")
    wc, wp = _post_f64(mixed.cpu().numpy(), -2, 0.7)
    np.testing.assert_array_equal(coarse.cpu().numpy(), wc)
    np.testing.assert_array_equal(pitchf.cpu().numpy(), wp.astype(np.float32))


@pytest.fixture(scope="module")
def vc():
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    return VC(40000, Config(DEV), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(9), DEV))


@pytest.mark.parametrize("method", ["hybrid[swipe]", "hybrid[rmvpe+swipe]", "hybrid[pm+swipe+swipe]"])
def test_vc_hybrid_is_the_mix_of_the_members_raw_tracks(vc, method):
    """VC.f0_device("hybrid[...]"): every member reads the f32 signal divided by its 0.999 |x| quantile (pm
    promoted to f64), contributes its raw track, and the mix goes through the f64 post."""
    from rvc_amd.pm import PitchPM
    from rvc_amd.swipe import SwipeAMD
    x = np.pad(synthetic.synthetic_audio(1.5, seed=31).astype(np.float32), (16000, 16000), mode="reflect")
    xp = torch.from_numpy(x).to(DEV)
    p_len = len(x) // 160
    xn = torch.from_numpy(x / np.quantile(np.abs(x), 0.999)).to(DEV)
    raw = {"swipe": lambda: SwipeAMD(DEV).f0(xn),
           "rmvpe": lambda: vc.rmvpe.f0_device(xn, 0.03, 0.0, want_f0=True)[2],
           "pm": lambda: torch.from_numpy(_pm_padded(PitchPM(DEV).to_pitch_ac(xn.double()).cpu().numpy(),
                                                     p_len)).to(DEV)}
    members = f0mix.parse_hybrid(method)
    want = f0mix.mix([raw[m]() for m in members], p_len).cpu().numpy()
    assert (want > 0).mean() > 0.3
    coarse, pitchf = vc.f0_device(xp, 2, method, True, 0.5)
    assert coarse.shape == pitchf.shape == (p_len,)
    wc, wp = _post_f64(want, 2, 0.5)
    np.testing.assert_array_equal(pitchf.cpu().numpy(), wp.astype(np.float32))
    np.testing.assert_array_equal(coarse.cpu().numpy(), wc)


def _pm_padded(f0, p_len):
    pad = (p_len - len(f0) + 1) // 2
    return np.pad(f0, [[pad, p_len - len(f0) - pad]], mode="constant")


def test_vc_hybrid_names_the_member_it_refuses(vc):
    xp = torch.zeros(16000, device=DEV)
    with pytest.raises(NotImplementedError, match="harvest"):
        vc.f0_device(xp, 0, "hybrid[rmvpe+harvest]")
    with pytest.raises(NotImplementedError, match="harvest"):
        vc.pipeline(None, None, 0, np.zeros(16000), 0, "hybrid[harvest]", "", 0.0, 1, 3, 1, "v2", 0.33, 64, False, 1,
                    ".pth", ".pt")
    with pytest.raises(NotImplementedError):
        vc.pipeline(None, None, 0, np.zeros(16000), 0, "swipe", "", 0.0, 1, 3, 1, "v2", 0.33, 64, False, 1,
                    ".pth", ".pt", f0_onnx=True)
    with pytest.raises(NotImplementedError):
        vc.f0_device(xp, 0, "dio")


def test_extract_forms(vc):
    """FeatureInputAMD.compute_f0: "swipe" -> f32 [1 + N // 160]; "hybrid[...]" -> no normalisation, f64
    [N // 160] (extract.py:132-147); absent methods keep raising."""
    from rvc_amd.extract import FeatureInputAMD
    from rvc_amd.swipe import SwipeAMD
    x = synthetic.synthetic_audio(1.5, seed=31).astype(np.float32)[:23999]
    fi = FeatureInputAMD(device=DEV, rmvpe=vc.rmvpe)
    sw = fi.compute_f0(x, "swipe")
    assert sw.dtype == np.float32 and sw.shape == (1 + x.size // 160,)
    xd = torch.from_numpy(x).to(DEV)
    np.testing.assert_array_equal(sw, SwipeAMD(DEV).f0(xd).cpu().numpy())
    p_len = x.size // 160
    got = fi.compute_f0(x, "hybrid[rmvpe+swipe]")
    assert got.dtype == np.float64 and got.shape == (p_len,)
    want = f0mix.mix([vc.rmvpe.f0_device(xd, 0.03, 0.0, want_f0=True)[2], SwipeAMD(DEV).f0(xd)], p_len)
    np.testing.assert_array_equal(got, want.cpu().numpy())
    one = fi.compute_f0(x, "hybrid[swipe]")
    assert one.shape == (p_len,)
    np.testing.assert_array_equal(one, f0mix.mix([SwipeAMD(DEV).f0(xd)], p_len).cpu().numpy())
    with pytest.raises(NotImplementedError):
        fi.compute_f0(x, "harvest")
    with pytest.raises(NotImplementedError, match="harvest"):
        fi.compute_f0(x, "hybrid[rmvpe+harvest]")
