"""rmvpe-legacy f0 on the device (get_f0_rmvpe(legacy=True), convert.py:248-255; infer_from_audio_with_pitch,
RMVPE.py:228-234): rmvpe with the decoded f0 outside 50..1100 Hz zeroed before shift and autotune, against the
reference's recorded output (tests/golden/rmvpe_legacy.npz, make_golden_mangio.py)."""
import ctypes

import numpy as np
import pytest
import torch

import mangio_ref
from rvc_amd import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_LEN = 75
HZ = 1e-2  # tests/test_gpu_rmvpe.py's bound on the raw track
HYBRID = "hybrid[mangio-crepe-tiny+rmvpe-legacy]"


@pytest.fixture(scope="module")
def setup(golden):
    from rvc_amd.crepe import CrepeAMD
    from rvc_amd.extract import FeatureInputAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    g = golden("rmvpe_legacy")
    rm = RMVPEAMD(synthetic.rmvpe_state_dict(int(g["seeds"][0])), DEV)
    m = CrepeAMD(synthetic.crepe_state_dict(int(g["seeds"][1]), "tiny"), "tiny", DEV)
    m.dither_fn = lambda T: g["hybrid_dither"][:T]
    cfg = Config(DEV)
    cfg.x_pad = 0
    vc = VC(40000, cfg, rmvpe=rm, crepe={"tiny": m})
    fi = FeatureInputAMD(device=DEV, rmvpe=rm, crepe={"tiny": m})
    return g, rm, vc, fi, torch.from_numpy(g["x"]).to(DEV)


def _check_track(legacy, plain, want):
    """Zero exactly where the reference's is; elsewhere the same run's plain rmvpe, bit for bit, within HZ of it."""
    assert legacy.dtype == np.float64 and legacy.shape == want.shape
    np.testing.assert_array_equal(legacy == 0, want == 0)
    keep = want != 0
    assert legacy[keep].tobytes() == plain[keep].tobytes()
    assert np.abs(legacy - want).max() < HZ, np.abs(legacy - want).max()
    assert np.count_nonzero((plain != 0) & ~keep) >= 10  # the filter bit: frames the plain track voices


def test_raw_track(setup):
    g, rm, vc, _, x = setup
    legacy = vc.f0_raw(x, "rmvpe-legacy", P_LEN).cpu().numpy()
    plain = vc.f0_raw(x, "rmvpe", P_LEN).cpu().numpy()
    vc.check_errors()
    assert np.abs(plain - g["plain"]).max() < HZ
    _check_track(legacy, plain, g["legacy"])
    assert (plain > 1100).sum() >= 5 and ((plain > 0) & (plain < 50)).sum() >= 5  # the filter bites on both sides


@pytest.mark.parametrize("variant", ["plain", "tune", "file"])
def test_get_f0_matches_reference(setup, variant):
    """Against the reference's get_f0, and against get_f0's tail (the oracle's, f64) on the device's own legacy track:
    the filter comes before autotune and shift (a frame shifted across a bound stays)."""
    g, rm, vc, _, x = setup
    pitch, autotune, strength, f0_file = mangio_ref.variants()[variant]
    coarse, pitchf = vc.f0_device(x, pitch, "rmvpe-legacy", autotune, strength, f0_file)
    c, f = coarse.cpu().numpy(), pitchf.cpu().numpy()
    ref_c, ref_f = g[f"vc:{variant}:coarse"], g[f"vc:{variant}:pitchf"]
    print(f"{variant}: max |pitchf - reference| {np.abs(f - ref_f).max():.3g} Hz, "
          f"coarse equal {np.mean(c == ref_c):.3f}")
    assert np.abs(f - ref_f).max() < HZ
    assert np.mean(c == ref_c) >= 0.99 and np.abs(c - ref_c).max() <= 1
    own_c, own_f = mangio_ref.get_f0(vc.f0_raw(x, "rmvpe-legacy", P_LEN).cpu().numpy(), pitch,
                                     strength if autotune else None, f0_file)
    assert f.tobytes() == own_f.astype(np.float32).tobytes()
    assert np.mean(c == own_c) >= 0.99 and np.abs(c - own_c).max() <= 1
    vc.check_errors()


def test_extraction_route(setup):
    g, rm, vc, fi, x = setup
    f0 = fi.compute_f0(g["x"], "rmvpe-legacy")
    _check_track(f0, fi.compute_f0(g["x"], "rmvpe"), g["fi_f0"])
    hy = fi.compute_f0(g["x"], "hybrid[rmvpe-legacy]", 160)
    np.testing.assert_array_equal(hy, np.interp(np.linspace(0, len(f0), P_LEN), np.arange(len(f0)), f0))


def test_hybrid_with_mangio_matches_reference(setup):
    """get_f0 of hybrid[mangio-crepe-tiny+rmvpe-legacy] at hop 64, within the looser of the members' bounds."""
    g, rm, vc, _, x = setup
    coarse, pitchf = vc.f0_device(x, 0, HYBRID, hop_length=64)
    c, f = coarse.cpu().numpy(), pitchf.cpu().numpy()
    vc.check_errors()
    print(f"hybrid: max |pitchf - reference| {np.abs(f - g['hybrid:pitchf']).max():.3g} Hz, "
          f"coarse equal {np.mean(c == g['hybrid:coarse']):.3f}")
    looser = np.maximum(HZ, 1e-3 + 1e-4 * np.abs(g["hybrid:pitchf"]))  # per frame: rmvpe's bound or mangio's
    assert (np.abs(f - g["hybrid:pitchf"]) <= looser).all()
    assert np.mean(c == g["hybrid:coarse"]) >= 0.99 and np.abs(c - g["hybrid:coarse"]).max() <= 1
    assert np.count_nonzero(f) >= 10


def test_batched_decode_and_pipeline_batch(setup):
    """rmvpe-legacy batches where rmvpe does: f0_device_batch with the range, and pipeline_device_batch on two copies of
    the signal against the per-clip pass, up to the batched launches' summation order (f0_device_batch's docstring;
    the bounds of tests/test_gpu_batch.py)."""
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.synth import SynthesizerAMD
    g, rm, _, _, x = setup
    rng = (50, 1100)
    _, _, f0_b = rm.f0_device_batch(torch.stack([x, x]), want_f0=True, f0_range=rng)
    _, _, f0_1 = rm.f0_device(x, want_f0=True, f0_range=rng)
    for b in range(2):
        np.testing.assert_array_equal((f0_b[b] == 0).cpu().numpy(), g["legacy"] == 0)
        assert (f0_b[b] - f0_1).abs().max().item() <= 1e-3 * f0_1.abs().max().item()
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(71), DEV)
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(48000, "v2", seed=73), DEV)
    cfg = Config(DEV)
    cfg.x_pad = 0  # the 0.75 s signal is shorter than the 1 s reflect padding of the default windows
    vc = VC(48000, cfg, rmvpe=rm)
    vc.seed = 40
    outs = vc.pipeline_device_batch(hub, net_g, 0, [x, x], 0, "v2", 0.33, f0_method="rmvpe-legacy")
    plain = vc.pipeline_device_batch(hub, net_g, 0, [x, x], 0, "v2", 0.33, f0_method="rmvpe")
    for b in range(2):
        vc.seed = 40 + b
        ref = vc.pipeline_device(hub, net_g, 0, x, 0, "v2", 0.33, f0_method="rmvpe-legacy")
        assert outs[b].shape == ref.shape
        rel = ((outs[b] - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()
        assert rel <= 1e-4, (b, rel)
        assert not torch.equal(outs[b], plain[b])  # the zeroed frames are heard
    vc.check_errors()


def test_decode_range_unbounded_is_rmvpe_decode(golden):
    """rvc_rmvpe_decode_range at (-inf, +inf) against rvc_rmvpe_decode, every bit of f0, coarse and pitchf, on the
    reference's known-answer salience (257 frames: three blocks, the last one partial), with and without the post
    steps; and at (50, 1100) it is that f0 with the frames outside zeroed before them."""
    g = golden("rmvpe")
    sal = torch.from_numpy(np.ascontiguousarray(g["kat_salience"].T)).to(DEV)  # [360][257]
    F = sal.shape[1]
    lib = _lib.load()
    rep = np.linspace(80.0, 1500.0, 40)
    posts = [None, ops.F0Post(0.5, None, 0, DEV), ops.F0Post(None, rep, 30, DEV), ops.F0Post(1.0, rep, 250, DEV)]
    inf = float("inf")

    def run(post, shift, rng):
        f0 = torch.empty(F, dtype=torch.float64, device=DEV)
        coarse = torch.empty(F, dtype=torch.int64, device=DEV)
        pitchf = torch.empty(F, device=DEV)
        pr = ops._post_ref(post, F)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        if rng is None:
            ops.check(lib.rvc_rmvpe_decode(p(sal), F, F, 0.03, shift, pr, p(f0), p(coarse), p(pitchf), None), "decode")
        else:
            ops.check(lib.rvc_rmvpe_decode_range(p(sal), F, F, 0.03, rng[0], rng[1], shift, pr, p(f0), p(coarse),
                                                 p(pitchf), None), "decode_range")
        torch.cuda.synchronize()
        return f0.cpu().numpy(), coarse.cpu().numpy(), pitchf.cpu().numpy()

    raw = run(None, 1.0, None)[0]
    out = (raw < 50) | (raw > 1100)
    assert ((raw > 0) & (raw < 50)).sum() >= 10 and (raw > 1100).sum() >= 10 and (~out).sum() >= 20
    for post in posts:
        for shift in (1.0, 2 ** (3 / 12)):
            a, b = run(post, shift, None), run(post, shift, (-inf, inf))
            for u, v in zip(a, b):
                assert u.tobytes() == v.tobytes()
            c = run(post, shift, (50.0, 1100.0))
            strength = post.autotune_strength if post is not None else None
            want = np.where(out, 0.0, raw)
            if strength is not None:
                from oracle.pipeline import autotune_f0
                want = autotune_f0(want, strength)
            want = want * shift
            if post is not None and post.rep is not None:
                n = min(len(rep), F - post.rep_off)
                want[post.rep_off: post.rep_off + n] = rep[:n]
            assert c[0].tobytes() == want.tobytes(), np.flatnonzero(c[0] != want)[:5]
            assert c[2].tobytes() == want.astype(np.float32).tobytes()
    # through the op wrapper too
    f0 = torch.empty(F, dtype=torch.float64, device=DEV)
    ops.rmvpe_decode(sal, F, F, 0.03, 1.0, f0, torch.empty(F, dtype=torch.int64, device=DEV),
                     torch.empty(F, device=DEV), None, (50, 1100))
    np.testing.assert_array_equal(f0.cpu().numpy(), np.where(out, 0.0, raw))
