"""fcpe-legacy f0 on the device (csrc/performer.hip, rvc_amd/fcpe_legacy.py): the FAVOR+ attention kernels against
the f64 restatement tests/fcpe_legacy_ref.py, the decoder with its range open, the model and one layer's attention
against the reference's own output on synthetic weights (tests/golden/fcpe_legacy*.npz; test_fcpe_legacy_cpu.py
pins the restatement to it), then the wiring: VC.f0_device, hybrid[...], FeatureInputAMD, ClipGraph, VC.pipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fcpe_legacy_ref
import fcpe_ref
from rvc_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "fcpe_legacy.npz"))
ATTN = np.load(os.path.join(HERE, "golden", "fcpe_legacy_attn.npz"))
CASES = ("a", "b", "c")
TILE = 32  # RVC_PERFORMER_TILE: the time tile of the key pass and of the query pass
D = 64


def _pv(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib_ops():
    from rvc_amd import _lib, ops
    return _lib.load(), ops


def case_args(c):
    hop, p_len, thr, seed, n_layers, out_bias = GOLD["args_" + c]
    return dict(hop=int(hop), p_len=int(p_len), thr=float(thr),
                ckpt=dict(seed=int(seed), n_layers=int(n_layers), out_bias=float(out_bias)))


def logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


_MODELS = {}


def model(c):
    from rvc_amd.fcpe_legacy import FcpeLegacyAMD
    key = tuple(sorted(case_args(c)["ckpt"].items()))
    if key not in _MODELS:
        _MODELS[key] = FcpeLegacyAMD(synthetic.fcpe_legacy_checkpoint(**dict(key)), DEV)
    return _MODELS[key]


_FCPE = []


def fcpe_model():
    from rvc_amd.fcpe import FcpeAMD
    if not _FCPE:
        _FCPE.append(FcpeAMD(synthetic.fcpe_checkpoint(n_layers=2), DEV))
    return _FCPE[0]


@pytest.fixture(scope="module")
def f64():
    return {c: np.load(os.path.join(HERE, "golden", f"fcpe_legacy_f64_{c}.npz")) for c in CASES}


# ---------------------------------------------------------------------------------------------- the op
def _inputs(g, B, H, T, scale):
    """q, k, v [B][H][T][64].  q and k are unit Gaussians (the size of a LayerNorm's output through a unit-gain
    linear) times ``scale`` times a per-frame amplitude between 0.15 and 1: at scale 6 the loud frames' exponents
    underflow, so that the + 1e-4 alone decides their q' (and their k' vanishes), while the quiet frames keep the
    queries in play.  Frame 0 is quiet in both; frame 1 has a loud query and a second key that still counts."""
    amp = 0.15 + 0.85 * torch.rand(2, B, H, T, 1, generator=g)
    amp[..., 0, :] = 0.15
    if T > 1:
        amp[0][..., 1, :], amp[1][..., 1, :] = 1.0, 0.25
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    return q * amp[0] * scale, k * amp[1] * scale, v


_PROJ = {}


def _proj(M):
    if M not in _PROJ:
        _PROJ[M] = synthetic.fcpe_legacy_checkpoint(seed=M, n_layers=1, n_chans=8, nb_features=M)["model"][
            "decoder._layers.0.attn.fast_attention.projection_matrix"]
    return _PROJ[M]


def _run_op(q, k, v, proj, ldc_pad=0, rows_pad=0):
    """The kernels on q, k, v [B][H][T][64] laid out as slices of one [B][3 * 64 H + rows_pad][T + ldc_pad] buffer
    -> (out [B][H][T][64] read from a NaN-filled [B][64 H + rows_pad][T + ldc_pad] buffer, that buffer)."""
    lib, ops = _lib_ops()
    B, H, T, _ = q.shape
    M, HC, ld = proj.shape[0], H * D, T + ldc_pad
    qkv = torch.zeros(B, 3 * HC + rows_pad, ld)
    for i, t in enumerate((q, k, v)):
        qkv[:, i * HC:(i + 1) * HC, :T] = t.permute(0, 1, 3, 2).reshape(B, HC, T)
    qkv = qkv.to(DEV)
    out = torch.full((B, HC + rows_pad, ld), float("nan"), device=DEV)
    need = lib.rvc_performer_work_bytes(B, H, T, M)
    assert need > 0
    work = torch.empty(need // 4, device=DEV)
    pd = proj.to(DEV).contiguous()
    step = HC * ld * 4
    plain = ldc_pad == 0 and rows_pad == 0  # 0 = the default strides
    ops.check(lib.rvc_performer_attention(_pv(qkv), ctypes.c_void_p(qkv.data_ptr() + step),
                                          ctypes.c_void_p(qkv.data_ptr() + 2 * step), _pv(pd), _pv(out), B, H, T, D, M,
                                          0 if plain else ld, (3 * HC + rows_pad) * ld,
                                          0 if plain else (HC + rows_pad) * ld, _pv(work), need, ops._stream()),
              "performer_attention")
    full = out.cpu()
    return full[:, :HC, :T].reshape(B, H, D, T).permute(0, 1, 3, 2), full


def _check_op(g, B, H, T, M, scale, pad):
    proj = _proj(M)
    q, k, v = _inputs(g, B, H, T, scale)
    want = fcpe_legacy_ref.attention(q.double(), k.double(), v.double(), proj)
    tol = 8 * float((fcpe_legacy_ref.attention(q, k, v, proj).double() - want).abs().max())
    # a kernel that ignored the queries could not pass: the output moves by more than 100 tol when every query is
    # replaced by their time mean.  (Not at T = 1, where a query is its own mean, nor at M = 1, where the one
    # feature's q' cancels between numerator and denominator: there the function itself does not read q.)
    if T > 1 and M > 1:
        blind = fcpe_legacy_ref.attention(q.double().mean(dim=2, keepdim=True).expand_as(q), k.double(), v.double(),
                                          proj)
        assert float((blind - want).abs().max()) > 100 * tol, (B, H, T, M, scale)
    got, full = _run_op(q, k, v, proj, *pad)
    again, _ = _run_op(q, k, v, proj, *pad)
    assert torch.equal(got, again)
    HC = H * D
    assert full[:, HC:].isnan().all() and full[:, :, T:].isnan().all()  # nothing written outside out
    assert not got.isnan().any()
    err = float((got.double() - want).abs().max())
    return err, tol


@pytest.mark.parametrize("B,H", [(1, 1), (1, 8), (2, 1), (2, 8)])
def test_performer_attention_matches_restatement(B, H):
    """The kernels against the restatement in f64; tolerance 8 x the error of the same restatement in f32 on the
    CPU on the same inputs (test_glu_dwconv_silu's rule: the margin is for the order of the sums).  M = 1, 16, 17,
    266, 272 for the padded feature columns; every T around the time tile of both passes; operand scales 0.5, 2
    and 6; B = 2 with padded batch and channel strides, q / k / v slices of one buffer.  Each input with T > 1 and
    M > 1 is first shown, on the CPU, to depend on its queries by more than 100 tol; two calls are bit-identical;
    the output buffer starts as NaN."""
    g = torch.Generator().manual_seed(1000 * B + H)
    worst = 0.0
    for M in (1, 16, 17, 266, 272):
        for T in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 7):
            for scale in (0.5, 2.0, 6.0):
                err, tol = _check_op(g, B, H, T, M, scale, (3, 5) if B == 2 else (0, 0))
                worst = max(worst, err / tol)
                assert err <= tol, (M, T, scale, err, tol)
    print(f"B={B} H={H}: worst err / tol {worst:.3f}")


def test_performer_attention_many_tiles_per_block():
    """T = 32 * 32 + 33 frames: more than 32 time tiles, so a key-pass block walks two tiles and the partials of 17
    blocks per head are reduced."""
    g = torch.Generator().manual_seed(7)
    err, tol = _check_op(g, 1, 8, TILE * 32 + 33, 266, 0.5, (0, 0))
    print(f"err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_performer_attention_rejects_without_launch():
    lib, ops = _lib_ops()
    T, M = 40, 266
    x = torch.zeros(3 * 512, T, device=DEV)
    out = torch.full((512, T), float("nan"), device=DEV)
    proj = torch.zeros(272, 64, device=DEV)
    need = lib.rvc_performer_work_bytes(1, 8, T, M)
    work = torch.empty(need // 4, device=DEV)

    def call(D_=64, M_=M, nbytes=need):
        return lib.rvc_performer_attention(_pv(x), _pv(x), _pv(x), _pv(proj), _pv(out), 1, 8, T, D_, M_, 0, 0, 0,
                                           _pv(work), nbytes, ops._stream())

    for kw in (dict(D_=32), dict(D_=128), dict(M_=0), dict(M_=273), dict(nbytes=need - 4)):
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert out.isnan().all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.isnan().any()


# ---------------------------------------------------------------------------------------------- decode
def test_decode_crafted_latents_range_open():
    """The legacy decode (rvc_fcpe_decode with f0_min = 0 and f0_max = FLT_MAX): a lone peak below 50 Hz and one
    above 1100 Hz come back unclamped and voiced; a confidence exactly at 0.03 gives 0 and one f32 step above it
    is voiced.  Voicing exact, values within test_decode_crafted_latents' rtol."""
    m = model("c")
    cent = m.cent_table.cpu().numpy()
    thr = np.float32(0.03)
    rng = np.random.default_rng(12)
    f = 10 * 2 ** (cent.astype(np.float64) / 1200)
    below, above = int(np.flatnonzero(f < 49.5)[-1]), int(np.flatnonzero(f > 1110)[0])
    lat = np.full((6, 360), 1e-6, np.float32)
    lat[0, below], lat[1, above], lat[2, 0], lat[3, 359] = 0.9, 0.9, 0.8, 0.8
    lat[4] = lat[5] = (rng.random(360) * 1e-3).astype(np.float32)
    lat[4, 150], lat[5, 150] = thr, np.nextafter(thr, np.float32(1))
    want = fcpe_legacy_ref.decode(lat, cent, thr)
    assert 40 < want[0] < 49.6 and 1110 < want[1] < 1200 and want[2] < 33.5 and want[3] > 1900
    assert want[4] == 0 and want[5] > 0
    clamped = fcpe_ref.decode(lat, cent, thr, 50, 1100)
    assert clamped[0] == 0 and clamped[1] == 1100
    got = m.decode(torch.from_numpy(np.ascontiguousarray(lat.T)).to(DEV), float(thr)).cpu().numpy()
    rtol = np.log(2) / 1200 * 9151 * 20 * 2.0 ** -24 + 4 * 2.0 ** -24
    np.testing.assert_array_equal(got > 0, want > 0)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


# ---------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("c", CASES)
def test_model_matches_reference(c, f64):
    """Against the reference on the same synthetic weights (12 layers in a and b, 2 in c).  With e = max
    |logit(latent32) - logit(latent64)| of the fixture (the reference's own f32 error): logits within 8 e of the f64
    run; argmax and voicing equal on every frame; the final f0 within 8 x the fixture's max rel |f0_32 - f0_64|;
    two calls bit-identical."""
    a = case_args(c)
    m = model(c)
    assert m.n_layers == a["ckpt"]["n_layers"]
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
    got = m.f0(x, a["p_len"], a["hop"], a["thr"])
    again = m.f0(x, a["p_len"], a["hop"], a["thr"])
    assert got.dtype == torch.float64 and torch.equal(got, again)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got > 0, want > 0)
    f0m = m.decode(torch.from_numpy(np.ascontiguousarray(lat.T)).to(DEV), a["thr"])
    np.testing.assert_array_equal(fcpe_ref.resize(f0m.cpu().numpy(), a["p_len"]) > 0, GOLD["f0m64_" + c] > 0)
    assert float(f0m.max()) > 1100  # no range: the fixtures hold voiced frames above VC's f0_max
    nz = want > 0
    tol = 8 * float(np.abs(GOLD["f0_32_" + c][nz] / want[nz] - 1).max())
    rel = float(np.abs(got[nz] / want[nz] - 1).max())
    print(f"{c}: f0 rel err {rel:.3e} tol {tol:.3e}")
    assert rel <= tol


def test_one_layer_attention_matches_reference():
    """Layer 0's attention through the real launch sequence, T = 51.  rvc_layernorm_cf on the layer's pinned input
    gives the reference's LayerNorm output (the fixture's ``x``) within 8 f32 roundings of its largest value; the
    QKV conv, the attention kernels and to_out on that ``x`` give the reference's f64 output within 8 x the
    reference's own f32 error |out32 - out64|."""
    _, ops = _lib_ops()
    m = model("c")
    L = m.layers[0]
    x, out64 = ATTN["x"], ATTN["out64"]
    T = x.shape[0]
    buf = m._buffers(T, torch.device(DEV, torch.cuda.current_device()))
    pre = torch.from_numpy(np.ascontiguousarray(ATTN["pre"].T)).to(DEV)
    n = torch.empty(512, T, device=DEV)
    ops.layernorm_cf(pre, None, L["norm"][0], L["norm"][1], n, 1, 512, T)
    ln_err = float(np.abs(n.cpu().numpy().T.astype(np.float64) - x).max())
    ln_tol = 8 * 2.0 ** -24 * float(np.abs(x).max())
    print(f"layernorm err {ln_err:.3e} tol {ln_tol:.3e}")
    assert ln_err <= ln_tol
    xd = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    out = torch.full((512, T), float("nan"), device=DEV)
    with ops.precision("fp32x6"):
        m.self_attention(L, xd, buf, out)
    err = float(np.abs(out.cpu().numpy().T.astype(np.float64) - out64).max())
    tol = 8 * float(np.abs(ATTN["out32"].astype(np.float64) - out64).max())
    print(f"attention err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_unsupported_models_raise():
    from rvc_amd.fcpe_legacy import FcpeLegacyAMD
    ck = synthetic.fcpe_legacy_checkpoint(n_layers=1)
    ck["config"]["model"]["confidence"] = True
    with pytest.raises(NotImplementedError, match="confidence"):
        FcpeLegacyAMD(ck, DEV)


# ---------------------------------------------------------------------------------------------- wiring
def _models(sr, version, seed, rmvpe=False):
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    from rvc_amd.synth import SynthesizerAMD
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(sr, version, seed=seed), DEV)
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(seed + 1), DEV)
    vc = VC(sr, Config(DEV), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(seed + 2), DEV) if rmvpe else None,
            fcpe=fcpe_model(), fcpe_legacy=model("c"))
    return vc, hub, net_g


def _pm_post(f0, pitch, post, p_len):
    lib, ops = _lib_ops()
    coarse = torch.empty(p_len, dtype=torch.int64, device=DEV)
    pitchf = torch.empty(p_len, device=DEV)
    ops.check(lib.rvc_pm_post(_pv(f0), p_len, p_len, float(2.0 ** (pitch / 12)), ops._post_ref(post, p_len),
                              _pv(coarse), _pv(pitchf), ops._stream()), "pm_post")
    return coarse, pitchf


def test_f0_device_equals_pm_post_of_f0():
    """vc.f0_device(xp, 2, "fcpe-legacy") = rvc_pm_post applied to FcpeLegacyAMD.f0 at threshold 0.03 (hop 64 by
    default and a given one), bit for bit, plain and with autotune and an f0 file; a VC without the model raises."""
    from rvc_amd import ops
    from rvc_amd.pipeline import VC, Config, f0_override
    m = model("c")
    vc = VC(40000, Config(DEV), fcpe=fcpe_model(), fcpe_legacy=m)
    xp = torch.from_numpy(np.pad(GOLD["x_a"], (16000, 16000), mode="reflect")).to(DEV)
    p_len = xp.numel() // 160
    inp_f0 = np.array([[0.10, 100.0], [0.30, 220.0], [0.45, 0.0], [0.60, 330.0]])
    rep, off = f0_override(inp_f0, vc.x_pad)
    for hop in (64, 160):
        raw = m.f0(xp, p_len, hop, 0.03)
        assert float(raw.max()) > float(raw.min()) > 0  # post_process bridges the unvoiced runs
        for pitch, strength, f0_file in ((2, None, None), (2, 0.7, inp_f0), (-3, None, inp_f0)):
            coarse, pitchf = vc.f0_device(xp, pitch, "fcpe-legacy", strength is not None, strength or 1.0, f0_file,
                                          hop_length=hop)
            post = None
            if strength is not None or f0_file is not None:
                post = ops.F0Post(strength, *((rep, off) if f0_file is not None else (None, 0)), xp.device)
            wc, wp = _pm_post(raw, pitch, post, p_len)
            assert coarse.dtype == torch.int64 and pitchf.dtype == torch.float32
            assert torch.equal(coarse, wc) and torch.equal(pitchf, wp)
            assert int(coarse.max()) > 1
    bare = VC(40000, Config(DEV), fcpe=fcpe_model())
    with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy="):
        bare.f0_device(xp, 0, "fcpe-legacy")
    with pytest.raises(NotImplementedError, match="fcpe-legacy.*fcpe_legacy="):
        bare.f0_device(xp, 0, "hybrid[fcpe-legacy+swipe]")


def test_hybrid_with_fcpe_legacy_equals_mix_of_raw_tracks():
    from rvc_amd import f0mix
    from rvc_amd.pipeline import VC, Config
    m = model("c")
    vc = VC(40000, Config(DEV), fcpe_legacy=m)
    xp = torch.from_numpy(np.pad(GOLD["x_a"], (16000, 16000), mode="reflect")).to(DEV)
    p_len = xp.numel() // 160
    xn = f0mix.normalize(xp)
    tracks = [m.f0(xn, p_len, 64, 0.03), vc._swipe(DEV).f0(xn)]
    assert torch.equal(vc.f0_raw(xn, "fcpe-legacy", p_len), tracks[0])
    want = _pm_post(f0mix.mix(tracks, p_len), 1, None, p_len)
    got = vc.f0_device(xp, 1, "hybrid[fcpe-legacy+swipe]")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert "fcpe-legacy" not in VC.HYBRID_EXTRA and "fcpe-legacy" not in f0mix.MEMBERS


def test_feature_input_compute_f0():
    from rvc_amd.extract import FeatureInputAMD
    m = model("c")
    fi = FeatureInputAMD(device=DEV, fcpe_legacy=m)
    x = GOLD["x_b"]
    for hop in (160, 64):
        got = fi.compute_f0(x, "fcpe-legacy", hop)
        want = m.f0(torch.from_numpy(x).to(DEV), x.size // 160, hop, 0.03).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (x.size // 160,)
        np.testing.assert_array_equal(got, want)
    assert fi.compute_f0(x, "hybrid[fcpe-legacy+swipe]", 64).shape == (x.size // 160,)
    with pytest.raises(NotImplementedError, match="fcpe-legacy"):
        FeatureInputAMD(device=DEV).compute_f0(x, "fcpe-legacy", 64)


def test_clip_graph_fcpe_legacy_replay_matches_eager():
    """Captured and replayed on two inputs = the eager pipeline_device, bit for bit: nothing on the fcpe-legacy path
    reads back to the host."""
    from rvc_amd.graph import ClipGraph
    vc, hub, net_g = _models(48000, "v2", 7)
    a1 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1001)).to(DEV)
    a2 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1002)).to(DEV)
    g = ClipGraph(vc, hub, net_g, 0, a1.numel(), f0_method="fcpe-legacy")
    for audio, seed in ((a1, 5), (a2, 5), (a1, 5)):
        got = g(audio, seed).clone()
        torch.cuda.synchronize()
        vc.seed = seed
        ref = vc.pipeline_device(hub, net_g, 0, audio, 0, "v2", 0.33, None, 0.0, "fcpe-legacy")
        assert got.shape == ref.shape
        assert torch.equal(got, ref), float((got - ref).abs().max())


def test_pipeline_end_to_end():
    """VC.pipeline(..., "fcpe-legacy", ...) on a 1.5 s clip returns what "rmvpe" does in length and dtype; a VC
    without the model still raises, naming the method."""
    from rvc_amd.pipeline import VC, Config
    vc, hub, net_g = _models(32000, "v1", 141, rmvpe=True)
    audio = synthetic.synthetic_audio(1.5, seed=9)
    args = ("", 0.0, 1, 3, 1, "v1", 0.33, 64, False, 1, ".pth", ".pt")
    out = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "fcpe-legacy", *args)
    ref = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "rmvpe", *args)
    assert out.shape == ref.shape and out.dtype == ref.dtype and np.isfinite(out).all() and np.abs(out).max() > 0
    hyb = vc.pipeline(hub, net_g, 0, audio.copy(), 0, "hybrid[fcpe-legacy+swipe]", *args)
    assert hyb.shape == ref.shape
    bare = VC(32000, Config(DEV), rmvpe=vc.rmvpe)
    for method in ("fcpe-legacy", "hybrid[fcpe-legacy+rmvpe]"):
        with pytest.raises(NotImplementedError, match="fcpe-legacy"):
            bare.pipeline(hub, net_g, 0, audio.copy(), 0, method, *args)
