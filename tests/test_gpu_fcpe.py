"""fcpe f0 on the device (csrc/fcpe.hip, rvc_amd/fcpe.py): the new ops against torch on the CPU in f64 and the
numpy restatement tests/fcpe_ref.py, the model against the reference's own output on synthetic weights
(tests/golden/fcpe.npz, fcpe_f64_<case>.npz; test_fcpe_cpu.py pins the restatement to it), then the wiring:
VC.f0_device, hybrid[...], FeatureInputAMD, ClipGraph and VC.pipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fcpe_ref
from rvc_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "fcpe.npz"))
CASES = ("a", "b", "c")
TILE = 256  # RVC_GLU_DW_TILE


def _pv(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib_ops():
    from rvc_amd import _lib, ops
    return _lib.load(), ops


def case_args(c):
    hop, p_len, thr, f0_min, f0_max, seed, n_layers, harm = GOLD["args_" + c]
    return dict(hop=int(hop), p_len=int(p_len), thr=float(thr), f0_min=int(f0_min), f0_max=int(f0_max),
                ckpt=dict(seed=int(seed), n_layers=int(n_layers), use_harmonic_emb=bool(harm)))


def logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


_MODELS = {}


def model(c):
    from rvc_amd.fcpe import FcpeAMD
    key = tuple(sorted(case_args(c)["ckpt"].items()))
    if key not in _MODELS:
        _MODELS[key] = FcpeAMD(synthetic.fcpe_checkpoint(**dict(key)), DEV)
    return _MODELS[key]


@pytest.fixture(scope="module")
def f64():
    return {c: np.load(os.path.join(HERE, "golden", f"fcpe_f64_{c}.npz")) for c in CASES}


# ---------------------------------------------------------------------------------------------- ops
def _glu_ref(x, w, b, K, dtype):
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    H = w.shape[0]
    return F.silu(F.conv1d(F.glu(x, dim=1), w[:, None, :], b, padding=K // 2, groups=H))


@pytest.mark.parametrize("K", [3, 31])
@pytest.mark.parametrize("B,H", [(1, 8), (3, 8), (1, 1024), (3, 1024)])
def test_glu_dwconv_silu(B, H, K):
    """Every T around the kernel's paths (one frame, below / at / above K's half-width, the time tile - 1 / tile /
    tile + 1, two tiles and a tail) against torch in f64; tolerance 8 x the error of the same composition in f32
    on the CPU (tap order and expf differ), measured here."""
    lib, ops = _lib_ops()
    g = torch.Generator().manual_seed(100 * H + 10 * B + K)
    for T in (1, 15, 16, 31, TILE - 1, TILE, TILE + 1, 2 * TILE + 7):
        x = torch.randn(B, 2 * H, T, generator=g) * 2
        w = torch.randn(H, K, generator=g) / K ** 0.5
        b = torch.randn(H, generator=g) * 0.1
        want = _glu_ref(x, w, b, K, torch.float64)
        tol = 8 * float((_glu_ref(x, w, b, K, torch.float32).double() - want).abs().max())
        y = torch.full((B, H, T), float("nan"), device=DEV)
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
        ops.check(lib.rvc_glu_dwconv_silu(_pv(xd), _pv(wd), _pv(bd), _pv(y), B, H, T, K, ops._stream()),
                  "glu_dwconv_silu")
        err = float((y.cpu().double() - want).abs().max())
        print(f"B={B} H={H} K={K} T={T}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (T, err, tol)


@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("T", [1, 2, 151])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_groupnorm_act(C, T, offset):
    """GroupNorm(4, C) + LeakyReLU(0.01) against F.group_norm in f64.  With the common offset 1e3 the inputs'
    own f32 spacing is 6e-5 on a unit spread, and a variance taken by cancellation in f32 would be lost
    altogether; the bound is 8 x the f32 rounding of the output (|y| <= ~6) plus that of the affine terms."""
    lib, ops = _lib_ops()
    G, B = 4, 2
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(B, C, T, generator=g) + offset
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    want = F.leaky_relu(F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-5), 0.01)
    need = lib.rvc_groupnorm_work_bytes(B, G)
    work = torch.empty(need // 4, device=DEV)
    y = torch.full((B, C, T), float("nan"), device=DEV)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    ops.check(lib.rvc_groupnorm_act(_pv(xd), _pv(gd), _pv(bd), _pv(y), B, C, T, G, 1e-5, 0.01, _pv(work), need,
                                    ops._stream()), "groupnorm_act")
    err = float((y.cpu().double() - want).abs().max())
    tol = 8 * 2.0 ** -24 * max(1.0, float(want.abs().max()))
    print(f"C={C} T={T} offset={offset}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_decode_crafted_latents():
    """Crafted latents, no ties: argmax at bins 0, 3, 4, 355, 356, 359 (windows clamped at either end, a clamped
    bin counted again), a confidence exactly at the threshold (-> 0) and one f32 step above it, f0 just below
    f0_min (-> 0) and just above f0_max (-> f0_max); two batch elements.  Voicing exact, values within the
    decoder's f32 rounding (test_fcpe_cpu.RTOL's derivation: 20 roundings on <= 9151 cents, plus 4)."""
    lib, ops = _lib_ops()
    cent = synthetic.fcpe_checkpoint()["model"]["cent_table"].numpy()
    thr = np.float32(0.006)
    rng = np.random.default_rng(11)
    peaks = [0, 3, 4, 355, 356, 359, 100, 200, 300]
    T = len(peaks) + 6
    lat = (rng.random((T, 360)) * 1e-3).astype(np.float32)
    for t, c in enumerate(peaks):
        lat[t, c] = 0.5 + 0.01 * t
        for d in (1, 2):  # distinct neighbours so that a window shifted by one bin would show
            if c - d >= 0:
                lat[t, c - d] = 0.3 / d + 0.001 * t
            if c + d < 360:
                lat[t, c + d] = 0.25 / d + 0.002 * t
    t = len(peaks)
    lat[t] = lat[t + 1] = (rng.random(360) * 1e-4).astype(np.float32)
    lat[t, 150], lat[t + 1, 150] = thr, np.nextafter(thr, np.float32(1))
    # bins whose centre frequencies straddle f0_min = 50 and f0_max = 1100: a lone peak decodes to about its centre
    f = 10 * 2 ** (cent.astype(np.float64) / 1200)
    below, above = int(np.flatnonzero(f < 49.5)[-1]), int(np.flatnonzero(f > 1110)[0])
    for k, c in enumerate((below, below + 2, above - 2, above)):
        lat[t + 2 + k] = 1e-6
        lat[t + 2 + k, c] = 0.9
    both = np.stack([lat, lat[::-1]])  # [B][T][C]
    dev = torch.from_numpy(np.ascontiguousarray(both.transpose(0, 2, 1))).to(DEV)  # [B][C][T]
    cent_d = torch.from_numpy(cent).to(DEV)
    rtol = np.log(2) / 1200 * 9151 * 20 * 2.0 ** -24 + 4 * 2.0 ** -24
    # once with the range open (the model's own 32.7 Hz bin 0 is below 50: every window's value shows), once at
    # VC's 50..1100
    for f0_min, f0_max in ((10, 3000), (50, 1100)):
        want = fcpe_ref.decode(lat, cent, thr, f0_min, f0_max)
        assert want[t] == 0 and want[t + 1] > 0
        if f0_min == 50:
            assert want[t + 2] == 0 and 50 < want[t + 3] < 51 and 1080 < want[t + 4] < 1100 and want[t + 5] == 1100
        else:
            assert (want[:len(peaks)] > 0).all() and (want[t + 2:] > 0).all()
        out = torch.full((2, T), float("nan"), device=DEV)
        ops.check(lib.rvc_fcpe_decode(_pv(dev), _pv(cent_d), _pv(out), 2, 360, T, float(thr), float(f0_min),
                                      float(f0_max), ops._stream()), "fcpe_decode")
        got = out.cpu().numpy()
        for b, w in ((0, want), (1, want[::-1])):
            np.testing.assert_array_equal(got[b] > 0, w > 0)
            np.testing.assert_allclose(got[b], w, rtol=rtol, atol=0)
            assert (got[b][w == f0_max] == f0_max).all()


def _tracks(T):
    rng = np.random.default_rng(T)
    full = (rng.random(T) * 900 + 60).astype(np.float32)
    out = {"all_zero": np.zeros(T, np.float32)}
    one = np.zeros(T, np.float32)
    one[T // 3] = 220.5
    out["one_voiced"] = one
    mid = np.zeros(T, np.float32)
    mid[T // 3: 2 * T // 3] = full[T // 3: 2 * T // 3]
    out["middle"] = mid  # zeros at both ends: the first and last voiced values are held
    iso = full.copy()
    iso[rng.random(T) < 0.2] = 0
    iso[5] = iso[T - 6] = 0
    out["isolated_zeros"] = iso
    out["all_voiced"] = full
    return out


@pytest.mark.parametrize("hop", [64, 160])
@pytest.mark.parametrize("T", [151, 1300])
def test_post_matches_restatement(T, hop):
    """rvc_fcpe_post against fcpe_ref.post (which test_fcpe_cpu pins to torch and the reference): voicing exact,
    values within 1e-12 relative (f64).  T = 1300 gives every thread of the one block more than one frame."""
    from rvc_amd.fcpe import FcpeAMD
    for name, f0 in _tracks(T).items():
        for p_len in (T - 1, T, 2 * T + 3, T // 2):
            want = fcpe_ref.post(f0, p_len, hop)
            got = FcpeAMD.post(torch.from_numpy(f0).to(DEV), p_len, hop).cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (p_len,)
            np.testing.assert_array_equal(got > 0, want > 0, err_msg=f"{name} p_len={p_len}")
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"{name} p_len={p_len}")
            if name == "all_zero":
                assert not got.any()
            if name == "one_voiced":
                assert (got == got[0]).all() and (got[0] == 220.5 or got[0] == 0)


@pytest.mark.parametrize("c", ["a", "b"])
def test_mel_matches_reference(c, f64):
    """rvc_fcpe_mel against the reference's f64 mel within 4 x the reference's own f32 error (the fixture's
    max |mel32 - mel64|; the margin is for the order of the 513-term sums); N = 24000 and 23999; the last frame
    is a copy of the one before."""
    m = model(c)
    x = torch.from_numpy(GOLD["x_" + c]).to(DEV)
    mel64 = f64[c]["mel64"]  # [T][128]
    tol = 4 * float(np.abs(GOLD["mel32_" + c].astype(np.float64) - mel64).max())
    got = m.mel(x).cpu().numpy().T
    assert got.shape == mel64.shape == (x.numel() // 160 + 1, 128)
    err = float(np.abs(got - mel64).max())
    print(f"{c}: mel err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    np.testing.assert_array_equal(got[-1], got[-2])
    assert not np.array_equal(got[-2], got[-3])


def test_mel_batch_and_short_signal():
    """Two signals in one launch equal two launches; 433 samples (the shortest accepted) runs, 432 raises."""
    lib, ops = _lib_ops()
    m = model("a")
    x = torch.from_numpy(np.stack([GOLD["x_a"][:4000], GOLD["x_a"][4000:8000]])).to(DEV)
    T = 4000 // 160 + 1
    out = torch.empty(2, 128, T, device=DEV)
    ops.check(lib.rvc_fcpe_mel(_pv(x), _pv(m.basis), _pv(out), 2, 4000, ops._stream()), "fcpe_mel")
    for b in range(2):
        assert torch.equal(out[b], m.mel(x[b].contiguous()))
    assert m.mel(x[0, :433].contiguous()).shape == (128, 3)
    with pytest.raises(ValueError, match="432"):
        m.mel(x[0, :432].contiguous())


# ---------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("c", CASES)
def test_model_matches_reference(c, f64):
    """Against the reference on the same synthetic weights.  With e = max |logit(latent32) - logit(latent64)| of
    the fixture (the reference's own f32 error): logits within 8 e of the f64 run; argmax and voicing equal on
    every frame; the final f0 within 8 x the fixture's max rel |f0_32 - f0_64|; two calls bit-identical."""
    a = case_args(c)
    m = model(c)
    x = torch.from_numpy(GOLD["x_" + c]).to(DEV)
    l64 = logit(f64[c]["latent64"])
    e = float(np.abs(logit(GOLD["latent32_" + c]) - l64).max())
    lat = m.latent(x).cpu().numpy().T
    assert lat.shape == l64.shape
    err = float(np.abs(logit(lat) - l64).max())
    print(f"{c}: logit err {err:.3e}, e {e:.3e} (bound {8 * e:.3e})")
    assert err <= 8 * e
    np.testing.assert_array_equal(lat.argmax(axis=1), l64.argmax(axis=1))
    want = GOLD["f0_64_" + c]
    got = m.f0(x, a["p_len"], a["hop"], a["thr"], a["f0_min"], a["f0_max"])
    again = m.f0(x, a["p_len"], a["hop"], a["thr"], a["f0_min"], a["f0_max"])
    assert got.dtype == torch.float64 and torch.equal(got, again)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got > 0, want > 0)
    f0m = m.decode(torch.from_numpy(np.ascontiguousarray(lat.T)).to(DEV), a["thr"], a["f0_min"], a["f0_max"])
    np.testing.assert_array_equal(fcpe_ref.resize(f0m.cpu().numpy(), a["p_len"]) > 0, GOLD["f0m64_" + c] > 0)
    nz = want > 0
    tol = 8 * float(np.abs(GOLD["f0_32_" + c][nz] / want[nz] - 1).max())
    rel = float(np.abs(got[nz] / want[nz] - 1).max())
    print(f"{c}: f0 rel err {rel:.3e} tol {tol:.3e}")
    assert rel <= tol


def test_unsupported_models_raise():
    from rvc_amd.fcpe import FcpeAMD
    ck = synthetic.fcpe_checkpoint(n_layers=1)
    ck["config_dict"]["model"]["conv_only"] = False
    with pytest.raises(NotImplementedError, match="conv_only"):
        FcpeAMD(ck, DEV)


# ---------------------------------------------------------------------------------------------- wiring
def _models(sr, version, seed, rmvpe=False):
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    from rvc_amd.synth import SynthesizerAMD
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(sr, version, seed=seed), DEV)
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(seed + 1), DEV)
    vc = VC(sr, Config(DEV), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(seed + 2), DEV) if rmvpe else None,
            fcpe=model("a"))
    return vc, hub, net_g


def _pm_post(f0, pitch, post, p_len):
    lib, ops = _lib_ops()
    coarse = torch.empty(p_len, dtype=torch.int64, device=DEV)
    pitchf = torch.empty(p_len, device=DEV)
    ops.check(lib.rvc_pm_post(_pv(f0), p_len, p_len, float(2.0 ** (pitch / 12)), ops._post_ref(post, p_len),
                              _pv(coarse), _pv(pitchf), ops._stream()), "pm_post")
    return coarse, pitchf


def test_f0_device_equals_pm_post_of_f0():
    """vc.f0_device(xp, 2, "fcpe") = rvc_pm_post applied to FcpeAMD.f0 at VC's settings (hop 64 by default and a
    given one, threshold 0.006, 50..1100), bit for bit, plain and with autotune and an f0 file."""
    from rvc_amd import ops
    from rvc_amd.pipeline import VC, Config, f0_override
    m = model("a")
    vc = VC(40000, Config(DEV), fcpe=m)
    xp = torch.from_numpy(np.pad(GOLD["x_a"], (16000, 16000), mode="reflect")).to(DEV)
    p_len = xp.numel() // 160
    inp_f0 = np.array([[0.10, 100.0], [0.30, 220.0], [0.45, 0.0], [0.60, 330.0]])
    rep, off = f0_override(inp_f0, vc.x_pad)
    for hop in (64, 160):
        raw = m.f0(xp, p_len, hop, 0.006, 50, 1100)
        assert float(raw.max()) > float(raw.min()) > 0  # post_process bridges the unvoiced runs
        for pitch, strength, f0_file in ((2, None, None), (2, 0.7, inp_f0), (-3, None, inp_f0)):
            coarse, pitchf = vc.f0_device(xp, pitch, "fcpe", strength is not None, strength or 1.0, f0_file,
                                          hop_length=hop)
            post = None
            if strength is not None or f0_file is not None:
                post = ops.F0Post(strength, *((rep, off) if f0_file is not None else (None, 0)), xp.device)
            wc, wp = _pm_post(raw, pitch, post, p_len)
            assert coarse.dtype == torch.int64 and pitchf.dtype == torch.float32
            assert torch.equal(coarse, wc) and torch.equal(pitchf, wp)
            assert int(coarse.max()) > 1
    with pytest.raises(NotImplementedError, match="fcpe-legacy"):
        vc.f0_device(xp, 0, "fcpe-legacy")
    with pytest.raises(NotImplementedError, match="fcpe-legacy"):
        vc.f0_device(xp, 0, "hybrid[fcpe-legacy+swipe]")


def test_hybrid_with_fcpe_equals_mix_of_raw_tracks():
    from rvc_amd import f0mix
    from rvc_amd.pipeline import VC, Config
    m = model("a")
    vc = VC(40000, Config(DEV), fcpe=m)
    xp = torch.from_numpy(np.pad(GOLD["x_a"], (16000, 16000), mode="reflect")).to(DEV)
    p_len = xp.numel() // 160
    xn = f0mix.normalize(xp)
    tracks = [m.f0(xn, p_len, 64, 0.006, 50, 1100), vc._swipe(DEV).f0(xn)]
    assert torch.equal(vc.f0_raw(xn, "fcpe", p_len), tracks[0])
    want = _pm_post(f0mix.mix(tracks, p_len), 1, None, p_len)
    got = vc.f0_device(xp, 1, "hybrid[fcpe+swipe]")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_feature_input_compute_f0():
    from rvc_amd.extract import FeatureInputAMD
    m = model("a")
    fi = FeatureInputAMD(device=DEV, fcpe=m)
    x = GOLD["x_b"]
    for hop in (160, 64):
        got = fi.compute_f0(x, "fcpe", hop)
        want = m.f0(torch.from_numpy(x).to(DEV), x.size // 160, hop).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (x.size // 160,)
        np.testing.assert_array_equal(got, want)
    assert fi.compute_f0(x, "hybrid[fcpe+swipe]", 64).shape == (x.size // 160,)
    with pytest.raises(NotImplementedError, match="fcpe-legacy"):
        fi.compute_f0(x, "fcpe-legacy", 64)


def test_clip_graph_fcpe_replay_matches_eager():
    """Captured and replayed on two inputs = the eager pipeline_device, bit for bit: nothing on the fcpe path
    reads back to the host."""
    from rvc_amd.graph import ClipGraph
    vc, hub, net_g = _models(48000, "v2", 7)
    a1 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1001)).to(DEV)
    a2 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1002)).to(DEV)
    g = ClipGraph(vc, hub, net_g, 0, a1.numel(), f0_method="fcpe")
    for audio, seed in ((a1, 5), (a2, 5), (a1, 5)):
        got = g(audio, seed).clone()
        torch.cuda.synchronize()
        vc.seed = seed
        ref = vc.pipeline_device(hub, net_g, 0, audio, 0, "v2", 0.33, None, 0.0, "fcpe")
        assert got.shape == ref.shape
        assert torch.equal(got, ref), float((got - ref).abs().max())


def test_pipeline_end_to_end():
    """VC.pipeline(..., "fcpe", ...) on a 1.5 s clip returns what "rmvpe" does in length and dtype; methods that
    stay off the device path raise, naming themselves."""
    vc, hub, net_g = _models(32000, "v1", 141, rmvpe=True)
    audio = synthetic.synthetic_audio(1.5, seed=9)
    args = ("", 0.0, 1, 3, 1, "v1", 0.33, 64, False, 1, ".pth", ".pt")
    out = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "fcpe", *args)
    ref = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "rmvpe", *args)
    assert out.shape == ref.shape and out.dtype == ref.dtype and np.isfinite(out).all() and np.abs(out).max() > 0
    hyb = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "hybrid[fcpe+swipe]", *args)
    assert hyb.shape == ref.shape
    for method in ("fcpe-legacy", "harvest", "hybrid[fcpe-legacy+rmvpe]"):
        with pytest.raises(NotImplementedError, match=method.split("[")[-1].split("+")[0]):
            vc.pipeline(hub, net_g, 0, audio.copy(), 0, method, *args)
    with pytest.raises(NotImplementedError, match="onnx|ONNX"):
        vc.pipeline(hub, net_g, 0, audio.copy(), 0, "fcpe", *args, f0_onnx=True)
