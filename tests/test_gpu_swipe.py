"""swipe f0 on the device (csrc/swipe.hip, rvc_amd/swipe.py) against the f64 numpy restatement
tests/swipe_ref.py and the reference's own f0 (tests/golden/swipe.npz; test_swipe_cpu.py pins the restatement
to it frame for frame), then through VC.f0_device, VC.pipeline, the clip stream and ClipGraph."""
import os

import numpy as np
import pytest
import torch

import swipe_ref
from rvc_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swipe.npz"))
NAMES = sorted(k[2:] for k in GOLD.files if k.startswith("x_"))


@pytest.fixture(scope="module")
def sw():
    from rvc_amd.swipe import SwipeAMD
    return SwipeAMD(DEV)


@pytest.mark.parametrize("n", [161, 700, 2049, 16037])
def test_strength_matches_restatement(sw, n):
    """S against the f64 restatement, max |dS| <= 1e-10: 5e4 x the spread between two f64 evaluation orders
    (2.2e-15) and 6e3 x below an all-f32 evaluation's error (6e-7).  The sizes are a two-frame signal, lengths
    around and just over the largest window, and a tail that is a multiple of neither 64 nor 160."""
    x = GOLD[f"x_slice{n}"]
    assert len(x) == n
    want = swipe_ref.strength(x)
    got = sw.strength(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == want.shape == (429, n // 160 + 1)
    err = float(np.abs(got - want).max())
    print(f"n={n}: max |dS| = {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_f0_matches_reference(sw, name):
    """f0 against the reference's: same length, frames that differ in any way (voicing or grid step) <= 1 %;
    silence and noise give all zeros."""
    x, want = GOLD["x_" + name], GOLD["f0_" + name]
    got = sw.f0(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = int((got != want).sum())
    print(f"{name}: {bad} of {len(want)} frames differ")
    assert bad <= 0.01 * len(want)
    if name in ("noise", "silence"):
        assert not got.any()


def test_pick_on_hand_built_strength(sw):
    """The pick on a hand-built S against the restatement's, exactly: threshold edge (0.2999 -> 0, exactly 0.3
    voiced), argmax at candidate 0 and at 428 (pc[0] both, as the reference), ties (first index; one pair inside
    a block's candidate range, one across two ranges), and peaks whose parabola maximum lands on chosen grid
    steps.  The steps are 5, 8 and 11: the argmax is a strict maximum over its left neighbour, so the parabola's
    vertex lies strictly inside the middle half of the 17-point grid and steps 0..3 and 13..16 cannot be the
    grid's argmax for any S (step 4 / 12 only at an exact tie with a neighbour).  66 frames: two blocks."""
    pc = swipe_ref.tables()[0]
    F = 66
    rng = np.random.default_rng(3)
    S = 0.05 * rng.random((429, F))

    def peak(col, i, step, height=0.6):
        tc = 1 / pc[i - 1:i + 2]
        x = (tc / tc[1] - 1) * 2 * np.pi
        lo = np.log2(pc[i - 1])
        grid = 2 ** np.arange(lo, np.log2(pc[i + 1]) + 1 / 12 / 64, 1 / 12 / 64)
        xv = (((1 / grid) / tc[1] - 1) * 2 * np.pi)[step]
        S[i - 1:i + 2, col] = height - 40.0 * (x - xv) ** 2

    S[:, 0] *= 0.1
    S[100, 0] = 0.2999
    S[:, 1] *= 0.1
    S[99:102, 1] = (0.2, 0.3, 0.25)
    S[0, 2] = 0.7
    S[428, 3] = 0.7
    S[50, 4] = S[53, 4] = S[300, 4] = 0.5  # a tie inside one candidate range and across ranges: the first index
    S[49, 4], S[51, 4] = 0.4, 0.45
    S[107, 5] = S[108, 5] = 0.55     # a tie across the boundary of two candidate ranges (27 per range)
    S[106, 5] = 0.5
    for col, (i, step) in enumerate([(200, 5), (200, 8), (200, 11), (1, 5), (427, 11), (215, 8), (216, 5)], start=6):
        peak(col, i, step)
    for col in range(13, F):         # ordinary frames, the last block's partial tile included
        peak(col, 20 + 6 * col, 5 + col % 7, 0.31 + 0.01 * col)
    want = swipe_ref.pick(S)
    got = sw.pick(torch.from_numpy(S).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert want[0] == 0 and want[1] > 0
    assert want[2] == want[3] == np.float32(pc[0])
    lo = np.log2(pc[199])
    assert [float(v) for v in want[6:9]] == [float(np.float32(2 ** (lo + s / 12 / 64))) for s in (5, 8, 11)]
    assert abs(want[4] / pc[50] - 1) < 0.01 and abs(want[5] / pc[107] - 1) < 0.01


def test_f0_device_post_matches_numpy():
    """VC.f0_device("swipe") with shift -2, autotune 0.7 and an f0 file against convert.py:308-323's numpy
    expressions applied in f32 to the device's raw f0: coarse and pitchf exact."""
    from rvc_amd.pipeline import VC, Config, f0_override
    vc = VC(40000, Config(DEV))
    x = np.pad(GOLD["x_speechlike"], (16000, 16000), mode="reflect")
    xp = torch.from_numpy(x).to(DEV)
    raw = vc._swipe(DEV).f0(xp).cpu().numpy()
    assert (raw > 0).sum() > 100
    inp_f0 = np.array([[0.10, 100.0], [0.30, 220.0], [0.45, 0.0], [0.60, 330.0]])
    rep, off = f0_override(inp_f0, vc.x_pad)
    for pitch, strength, f0_file in ((-2, 0.7, inp_f0), (0, None, None), (3, None, inp_f0)):
        coarse, pitchf = vc.f0_device(xp, pitch, "swipe", strength is not None, strength or 1.0, f0_file)
        wc, wp = swipe_ref.get_f0_post_f32(raw, pitch, strength, rep if f0_file is not None else None, off)
        np.testing.assert_array_equal(pitchf.cpu().numpy(), wp)
        np.testing.assert_array_equal(coarse.cpu().numpy(), wc)


def _models(sr, version, seed, rmvpe=False):
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    from rvc_amd.synth import SynthesizerAMD
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(sr, version, seed=seed), DEV)
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(seed + 1), DEV)
    vc = VC(sr, Config(DEV), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(seed + 2), DEV) if rmvpe else None)
    return vc, hub, net_g


@pytest.mark.parametrize("method", ["swipe", "hybrid[rmvpe+swipe]"])
def test_pipeline_vs_oracle(method):
    """VC.pipeline on a 5 s synthetic clip against the oracle pipeline fed the device's own raw f0 track, with
    the same noise: <= 1e-4 RMS, the project's waveform bar.  Pitch 0.  The device quantises the swipe f0 in
    f32 (as the reference does for its f32 array) and the oracle in f64: for this clip (synthetic_audio(5.0,
    seed=9)) both give the same coarse bins and pitchf on every frame of the restatement's f0 -- checked on the
    CPU when the test was written (seeds 9..12 all agree).  The hybrid track is f64 [p_len]; the oracle expects
    p_len + 1 frames and drops the last, so it is padded by one."""
    from oracle import contentvec as ocv
    from oracle import pipeline as opl
    from oracle import synth as osy
    from rvc_amd import f0mix, melbasis
    sr, version, seed = 32000, "v1", 141
    vc, hub, net_g = _models(sr, version, seed, rmvpe="rmvpe" in method)
    audio = synthetic.synthetic_audio(5.0, seed=9)
    noises = {}

    def noise(seg, kind, shape):
        if (seg, kind) not in noises:
            noises[(seg, kind)] = torch.randn(*shape, generator=torch.Generator().manual_seed(11 * seg + len(kind)))
        return noises[(seg, kind)]

    vc.noise_fn = lambda s, k, sh: noise(s, k, sh).to(DEV)
    out = vc.pipeline(hub, net_g, 0, audio.copy(), 0, method, "", 0.0, 1, 3, 1, version, 0.33, 64, False, 1, ".pth",
                      ".pt")
    xp, _ = vc.filt(torch.from_numpy(audio.astype(np.float32)).to(DEV), vc.t_pad)
    p_len = xp.numel() // 160
    if method == "swipe":
        track = vc._swipe(DEV).f0(xp).cpu().numpy().astype(np.float64)
    else:
        xn = f0mix.normalize(xp)
        mixed = f0mix.mix([vc.f0_raw(xn, m, p_len) for m in ("rmvpe", "swipe")], p_len)
        track = np.append(mixed.cpu().numpy(), 0.0)
    assert track.shape == (p_len + 1,) and (track > 0).mean() > 0.5
    ck = synthetic.make_synth_ckpt(sr, version, seed=seed)
    ref = opl.pipeline(ocv.load_weights(synthetic.make_contentvec_ckpt(seed + 1)), osy.load_weights(ck["weight"]),
                       None, torch.from_numpy(melbasis.mel_filterbank()), ck["config"], 0, audio, 0.0, version, 0.33,
                       noise, f0_track=track)
    assert out.shape == ref.shape
    err = float(np.sqrt(np.mean((out.astype(np.float64) - ref) ** 2)))
    print(f"{method}: waveform RMS error {err:.3e}")
    assert err < 1e-4, err


@pytest.mark.parametrize("method", ["swipe", "hybrid[rmvpe+swipe]"])
def test_stream_bit_identical_to_per_clip(method):
    """The new f0 forms inside the clip stream = pipeline_device per clip."""
    vc, hub, net_g = _models(32000, "v1", 151, rmvpe=True)
    xs = [torch.from_numpy(synthetic.synthetic_audio(3.0, seed=60 + i)).to(DEV) for i in range(2)]
    vc.seed = 3
    outs = vc.pipeline_device_stream(hub, net_g, 0, xs, 0, "v1", 0.33, f0_method=method)
    torch.cuda.synchronize()
    for k, x in enumerate(xs):
        vc.seed = 3 + k
        ref = vc.pipeline_device(hub, net_g, 0, x, 0, "v1", 0.33, f0_method=method)
        assert torch.equal(outs[k], ref)
    vc.check_errors()


def test_clip_graph_swipe_replay_matches_eager():
    from rvc_amd.graph import ClipGraph
    vc, hub, net_g = _models(48000, "v2", 7)
    a1 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1001)).to(DEV)
    a2 = torch.from_numpy(synthetic.synthetic_audio(3.0, seed=1002)).to(DEV)
    g = ClipGraph(vc, hub, net_g, 0, a1.numel(), f0_method="swipe")
    for audio, seed in ((a1, 5), (a2, 5), (a1, 5)):
        got = g(audio, seed).clone()
        torch.cuda.synchronize()
        vc.seed = seed
        ref = vc.pipeline_device(hub, net_g, 0, audio, 0, "v2", 0.33, None, 0.0, "swipe")
        assert got.shape == ref.shape
        assert torch.equal(got, ref), float((got - ref).abs().max())
    with pytest.raises(NotImplementedError):
        ClipGraph(vc, hub, net_g, 0, a1.numel(), f0_method="hybrid[swipe]")
