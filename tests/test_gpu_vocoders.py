"""The MRF-HiFi-GAN and RefineGAN decoders on the HIP path: the reference's own outputs (golden vectors), the three
new kernels against torch / numpy on the host, and the model-level properties the default decoder is held to.

Every test here fails on a tree without the feature: SynthesizerAMD refused these checkpoints at load, and the
kernels did not exist."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_util as vu
from rvc_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCODERS = ["MRF-HiFi-GAN", "RefineGAN"]


@pytest.fixture(scope="module")
def ops():
    from rvc_amd import ops as o
    return o


# ------------------------------------------------------------------ the reference's goldens
@pytest.mark.parametrize("name", vu.GOLDENS)
def test_infer_matches_reference_golden(golden, name):
    """Synthesizer(vocoder=...).infer of the reference (tests/golden/make_golden_vocoders.py) with its draws injected:
    the bars of tests/test_gpu_synth.py, and ``har`` within 4 x the reference's own float32-vs-float64 spread of the
    source module (floor 1e-6)."""
    from rvc_amd.synth import SynthesizerAMD
    g = golden(name)
    ck = synthetic.make_synth_ckpt(int(g["sr"]), str(g["version"]), seed=int(g["seed"]), vocoder=str(g["vocoder"]))
    net = SynthesizerAMD(ck, DEV)
    T = int(g["T"])
    z_noise, phase0, sine, adain = vu.golden_draws(g, net.adain_shapes(T))
    o, x_mask, (z, z_p, m_p, logs_p) = net.infer(
        torch.from_numpy(g["phone"]).to(DEV), torch.tensor([T], device=DEV), torch.from_numpy(g["pitch"]).to(DEV),
        torch.from_numpy(g["pitchf"]).to(DEV), torch.from_numpy(g["sid"]).to(DEV), z_noise=z_noise.to(DEV),
        sine_noise=sine.to(DEV), phase0=phase0.to(DEV), adain_noise=[a.to(DEV) for a in adain] or None)
    ph = phase0.clone()
    ph[:, 0] = 0
    har = net.harmonic_source(torch.from_numpy(g["pitchf"]).to(DEV).contiguous(), sine.to(DEV).contiguous(),
                              ph.to(DEV), T)
    torch.cuda.synchronize()
    errs = dict(m_p=vu.rms(m_p, g["m_p"]), logs_p=vu.rms(logs_p, g["logs_p"]), z_p=vu.rms(z_p, g["z_p"]),
                z=vu.rms(z, g["z"]), har=vu.rms(har, g["har"]), o=vu.rms(o, g["o"]))
    print(name, errs, "har_ref_spread", float(g["har_ref_spread"]))
    assert o.shape == (1, 1, g["har"].shape[-1])
    assert errs["m_p"] < 1e-5 and errs["logs_p"] < 1e-5 and errs["z_p"] < 1e-5 and errs["z"] < 1e-5
    assert errs["har"] < max(4 * float(g["har_ref_spread"]), 1e-6)
    assert errs["o"] < 1e-4


# ------------------------------------------------------------------ rvc_upsample_linear
def _ulp_distance(a, b):
    def key(x):  # f32 bits as integers ordered like the floats
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("Lin", [1, 2, 37])
@pytest.mark.parametrize("r", [2, 10, 12])
def test_upsample_linear_matches_torch(ops, r, Lin):
    """F.interpolate(F.leaky_relu(x, 0.2), scale_factor=r, mode="linear") to 2 ulp, written into the first C channels
    of a wider buffer whose other rows stay untouched."""
    B, C, extra = 2, 5, 3
    g = torch.Generator().manual_seed(100 * r + Lin)
    x = torch.randn(B, C, Lin, generator=g)
    want = F.interpolate(F.leaky_relu(x, 0.2), scale_factor=r, mode="linear").numpy()
    Lout = Lin * r
    buf = torch.full((B, C + extra, Lout), -7.0, device=DEV)
    ops.upsample_linear(x.to(DEV), r, out=buf, act=ops.ACT_LRELU, slope=0.2, y_bstride=(C + extra) * Lout)
    got = buf.cpu().numpy()
    assert want.shape == (B, C, Lout)
    assert _ulp_distance(got[:, :C], want).max() <= 2
    assert (got[:, C:] == -7.0).all()
    # no activation, contiguous output
    plain = ops.upsample_linear(x.to(DEV), r).cpu().numpy()
    assert _ulp_distance(plain, F.interpolate(x, scale_factor=r, mode="linear").numpy()).max() <= 2


def test_upsample_linear_several_blocks(ops):
    """More outputs per row than one block's tile (4096), rows 16-byte aligned (the vector store path) or not."""
    for Lin, r in ((700, 6), (1031, 2), (1723, 3), (2500, 2)):
        x = torch.randn(2, 3, Lin, generator=torch.Generator().manual_seed(Lin))
        want = F.interpolate(x, scale_factor=r, mode="linear").numpy()
        got = ops.upsample_linear(x.to(DEV), r).cpu().numpy()
        assert _ulp_distance(got, want).max() <= 2, (Lin, r)


# ------------------------------------------------------------------ rvc_adain
def test_adain_buffer_noise_matches_torch(ops):
    B, C, L = 2, 6, 131
    g = torch.Generator().manual_seed(9)
    x, n = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    w = torch.rand(C, generator=g) + 0.1
    want = F.leaky_relu(x + n * w[None, :, None], 0.2)
    out = torch.empty(B, C, L, device=DEV)
    ops.adain(x.to(DEV), w.to(DEV), out, noise=n.to(DEV), slope=0.2)
    assert (out.cpu() - want).abs().max().item() <= 1e-6


@pytest.mark.parametrize("n", [1, 255, 4 * 1024 + 3])
def test_adain_in_kernel_draw_equals_randn_buffer(ops, n):
    """The production form (noise drawn in the kernel) is bit-identical to the parity form reading a buffer that
    ops.randn filled with the same (seed, offset) -- per clip, each with its own seed; n = C*L over odd splits."""
    for C in (1, 3) if n % 3 == 0 else (1,):
        L = n // C
        B, seeds, off = 2, (17, 40), ops.off_adain(5)
        g = torch.Generator().manual_seed(n)
        x = torch.randn(B, C, L, generator=g).to(DEV)
        w = (torch.rand(C, generator=g) + 0.1).to(DEV)
        buf = torch.empty(B, C, L, device=DEV)
        for b in range(B):
            ops.randn(buf[b], seeds[b], off)
        a = torch.empty(B, C, L, device=DEV)
        c = torch.empty(B, C, L, device=DEV)
        ops.adain(x, w, a, noise=buf, slope=0.2)
        ops.adain(x, w, c, seeds=seeds, offset=off, slope=0.2)
        assert torch.equal(a, c)


def test_adain_accumulate_forms_the_mean(ops):
    B, C, L = 2, 4, 257
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(B, C, L, generator=g) for _ in range(3)]
    ns = [torch.randn(B, C, L, generator=g) for _ in range(3)]
    ws = [torch.rand(C, generator=g) + 0.1 for _ in range(3)]
    want = torch.stack([F.leaky_relu(x + n * w[None, :, None], 0.2) for x, n, w in zip(xs, ns, ws)]).mean(0)
    out = torch.full((B, C, L), 5.0, device=DEV)
    for j in range(3):
        ops.adain(xs[j].to(DEV), ws[j].to(DEV), out, noise=ns[j].to(DEV), slope=0.2, out_scale=1.0 / 3.0,
                  accumulate=j > 0)
    assert (out.cpu() - want).abs().max().item() <= 1e-6


# ------------------------------------------------------------------ rvc_harmonic_source
@pytest.mark.parametrize("linear,H", [(False, 9), (True, 1), (True, 9)])
def test_harmonic_source_multi_block_scan(ops, linear, H):
    """A scan over several blocks (L = 3 * chunk + 1 samples, upp = 1 so every sample has its own f0) at B = 2 against
    the float64 numpy restatement, to 1e-5 RMS."""
    chunk = int(ops._lib.load().rvc_harmonic_source_chunk())
    B, upp, sr = 2, 1, 40000
    T = 3 * chunk + 1
    rng = np.random.Generator(np.random.PCG64(H + 10 * linear))
    f0 = np.repeat(rng.uniform(80, 900, size=(B, T // 64 + 1)), 64, axis=1)[:, :T].astype(np.float32)
    f0[:, 1000:1500] = 0.0  # an unvoiced run
    phase0 = rng.uniform(0, 1, size=(B, H)).astype(np.float32)
    phase0[:, 0] = 0
    noise = rng.standard_normal((B, T * upp, H)).astype(np.float32)
    lin_w = rng.uniform(-1.2, 1.2, size=H).astype(np.float32).tolist()
    want = vu.np_harmonic_source(f0, phase0, noise, upp, sr, lin_w, 0.05, linear)
    har = torch.empty(B, T * upp, device=DEV)
    ops.harmonic_source(torch.from_numpy(f0).to(DEV), torch.from_numpy(phase0).to(DEV),
                        torch.from_numpy(noise).to(DEV), har, B, T, upp, H, float(sr), lin_w, 0.05, linear=linear)
    assert vu.rms(har, want) < 1e-5
    # the last block alone (its carry is the sum of everything before it)
    assert vu.rms(har[:, -chunk:], want[:, -chunk:]) < 1e-5


def test_harmonic_source_upsampled_frames(ops):
    """Frames upsampled by upp = 480 (nearest and linear), L a little over one block."""
    B, T, upp, sr, H = 2, 11, 480, 48000, 9
    rng = np.random.Generator(np.random.PCG64(4))
    f0 = rng.uniform(60, 500, size=(B, T)).astype(np.float32)
    f0[:, 3:5] = 0.0
    phase0 = rng.uniform(0, 1, size=(B, H)).astype(np.float32)
    phase0[:, 0] = 0
    noise = rng.standard_normal((B, T * upp, H)).astype(np.float32)
    lin_w = rng.uniform(-1.2, 1.2, size=H).astype(np.float32).tolist()
    for linear in (False, True):
        want = vu.np_harmonic_source(f0, phase0, noise, upp, sr, lin_w, -0.02, linear)
        har = torch.empty(B, T * upp, device=DEV)
        ops.harmonic_source(torch.from_numpy(f0).to(DEV), torch.from_numpy(phase0).to(DEV),
                            torch.from_numpy(noise).to(DEV), har, B, T, upp, H, float(sr), lin_w, -0.02, linear=linear)
        assert vu.rms(har, want) < 1e-5, linear


# ------------------------------------------------------------------ model-level properties
def _inputs(net, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    phone = torch.randn(B, net.emb_dim, T, generator=g).to(DEV)
    pitch = torch.randint(1, 255, (B, T), generator=g).to(DEV)
    nsff0 = (100 + 300 * torch.rand(B, T, generator=g))
    nsff0[:, T // 3: T // 2] = 0
    return phone, pitch, nsff0.to(DEV)


@pytest.fixture(scope="module")
def nets():
    from rvc_amd.synth import SynthesizerAMD
    return {v: SynthesizerAMD(synthetic.make_synth_ckpt(48000, "v2", seed=5, vocoder=v), DEV) for v in VOCODERS}


@pytest.mark.parametrize("vocoder", VOCODERS)
def test_device_noise_is_deterministic(nets, vocoder):
    net = nets[vocoder]
    T = 48
    phone = torch.randn(1, T, 768, generator=torch.Generator().manual_seed(0)).to(DEV)
    pitch = torch.randint(1, 255, (1, T), generator=torch.Generator().manual_seed(1)).to(DEV)
    pitchf = (torch.rand(1, T, generator=torch.Generator().manual_seed(2)) * 400).to(DEV)
    a = net.infer(phone, torch.tensor([T]), pitch, pitchf, 0, seed=7)[0]
    b = net.infer(phone, torch.tensor([T]), pitch, pitchf, 0, seed=7)[0]
    c = net.infer(phone, torch.tensor([T]), pitch, pitchf, 0, seed=8)[0]
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert a.shape == (1, 1, T * 480)
    assert torch.isfinite(a).all() and float(a.abs().max()) <= 1.0


@pytest.mark.parametrize("vocoder", VOCODERS)
def test_decode_batch_equals_single_clip_calls(nets, vocoder):
    """decode_batch over B = 2 clips equals two B = 1 calls bit for bit."""
    net = nets[vocoder]
    B, T, seeds = 2, 40, (11, 12)
    phone, pitch, nsff0 = _inputs(net, B, T, 5)
    z, _, _, gc = net.prior_batch(phone, pitch, 0, None, seeds)
    o = net.decode_batch(z, nsff0, gc, None, seeds)
    assert o.shape == (B, T * net.upp)
    for b in range(B):
        o1 = net.decode_batch(z[b:b + 1].contiguous(), nsff0[b:b + 1].contiguous(), gc, None, (seeds[b],))
        assert torch.equal(o[b], o1[0]), (b, (o[b] - o1[0]).abs().max().item())
    assert not torch.equal(o[0], o[1])


@pytest.mark.parametrize("vocoder", ["MRF HiFi-GAN", "RefineGAN"])
@pytest.mark.parametrize("sr", [32000, 48000])
def test_five_stage_v1_configs_run(vocoder, sr):
    """The five-stage v1 configs (and the MRF spelling with a space) load and run."""
    from rvc_amd.synth import SynthesizerAMD
    net = SynthesizerAMD(synthetic.make_synth_ckpt(sr, "v1", seed=6, vocoder=vocoder), DEV)
    T = 20
    phone, pitch, nsff0 = _inputs(net, 1, T, 8)
    o = net.infer_cf(phone[0].contiguous(), pitch[0].contiguous(), nsff0[0].contiguous(), 0, seed=3)[0]
    assert o.shape == (T * net.upp,)
    assert torch.isfinite(o).all() and float(o.abs().max()) <= 1.0 and float(o.abs().max()) > 1e-3


def test_no_f0_and_unknown_vocoders_stay_refused():
    from rvc_amd.synth import SynthesizerAMD
    ck = synthetic.make_synth_ckpt(40000, "v2", seed=6, vocoder="RefineGAN")
    ck["f0"] = 0
    with pytest.raises(NotImplementedError):
        SynthesizerAMD(ck, DEV)
    ck["f0"], ck["vocoder"] = 1, "BigVGAN"
    with pytest.raises(NotImplementedError, match="BigVGAN"):
        SynthesizerAMD(ck, DEV)


# ------------------------------------------------------------------ VC.pipeline
@pytest.fixture(scope="module")
def front():
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(71), DEV)
    rm = RMVPEAMD(synthetic.rmvpe_state_dict(72), DEV)
    return hub, VC(48000, Config(DEV), rmvpe=rm)


@pytest.mark.parametrize("vocoder", VOCODERS)
def test_pipeline_and_stream(front, nets, vocoder):
    """Two 2 s clips through VC.pipeline_device with each new vocoder, and through the clip stream: the stream equals
    the per-call pipeline bit for bit (as tests/test_gpu_batch.py holds the default decoder to)."""
    hub, vc = front
    net_g = nets[vocoder]
    xs = [torch.from_numpy(synthetic.synthetic_audio(2.0, seed=600 + i)).to(DEV) for i in range(2)]
    vc.seed = 40
    try:
        outs = vc.pipeline_device_stream(hub, net_g, 0, xs, 0, "v2", 0.33)
        torch.cuda.synchronize()
        for k, x in enumerate(xs):
            vc.seed = 40 + k
            ref = vc.pipeline_device(hub, net_g, 0, x, 0, "v2", 0.33)
            assert 0.95 * 2 * 48000 <= ref.numel() <= 2 * 48000 and torch.isfinite(ref).all()
            assert float(ref.abs().max()) > 1e-3
            assert outs[k].shape == ref.shape
            assert torch.equal(outs[k], ref), (k, (outs[k] - ref).abs().max().item())
    finally:
        vc.seed = 0
    vc.check_errors()


@pytest.mark.parametrize("vocoder", VOCODERS)
def test_pipeline_noise_fn_is_asked_for_the_new_kinds(front, nets, vocoder):
    """With a noise_fn the pipeline asks it for every draw of the decoder -- "z" and "sine" as ever, then "phase" and
    RefineGAN's "adain<k>" -- and the output no longer depends on the seed."""
    hub, vc = front
    net_g = nets[vocoder]
    x = torch.from_numpy(synthetic.synthetic_audio(2.0, seed=650)).to(DEV)
    asked = []

    def noise_fn(seg, kind, shape):
        asked.append((kind, tuple(shape)))
        g = torch.Generator().manual_seed(1000 * seg + len(asked))
        return (torch.rand if kind == "phase" else torch.randn)(*shape, generator=g).to(DEV)

    vc.noise_fn = noise_fn
    try:
        vc.seed = 1
        a = vc.pipeline_device(hub, net_g, 0, x, 0, "v2", 0.33)
        first, asked[:] = list(asked), []
        vc.seed = 2
        b = vc.pipeline_device(hub, net_g, 0, x, 0, "v2", 0.33)
    finally:
        vc.noise_fn, vc.seed = None, 0
    assert torch.equal(a, b) and asked == first
    T = first[0][1][2]  # frames of the padded segment
    assert first[0][1] == (1, net_g.inter, T) and T * net_g.upp >= a.numel()
    H = net_g.n_harm
    kinds = [k for k, _ in first]
    assert kinds == ["z", "sine", "phase"] + [f"adain{k}" for k in range(len(net_g.adain_shapes(T)))]
    assert first[1][1] == (1, T * net_g.upp, H) and first[2][1] == (1, H)
    assert [s for _, s in first[3:]] == [(1, C, L) for C, L in net_g.adain_shapes(T)]
    assert len(first) == (27 if vocoder == "RefineGAN" else 3)
