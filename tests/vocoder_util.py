"""Helpers shared by the MRF-HiFi-GAN / RefineGAN tests: the goldens' seeded draws and a float64 numpy
restatement of the per-sample harmonic source."""
import numpy as np
import torch

GOLDENS = ["mrf_48k_v2", "mrf_40k_v2", "refinegan_48k_v2", "refinegan_32k_v2"]


def draw(draw_seed: int, index: int, kind: str, shape) -> torch.Tensor:
    """The index-th draw of a golden run (tests/golden/make_golden_vocoders.py ``draw``)."""
    g = torch.Generator().manual_seed(draw_seed * 1000 + index)
    fn = torch.rand if kind == "rand" else torch.randn
    return fn(*shape, generator=g, dtype=torch.float32)


def golden_draws(g, adain_shapes):
    """(z_noise [1][inter][T], phase0 [1][H], sine_noise [1][L][H], [AdaIN draws [1][C][L]]) of golden ``g``: the
    reference draws z, then the source's torch.rand phases, its noise, then the AdaINs' in order."""
    ds, T = int(g["draw_seed"]), int(g["T"])
    L = g["har"].shape[-1]
    H = 9 if str(g["vocoder"]).startswith("MRF") else 1
    z_noise = draw(ds, 0, "randn", g["m_p"].shape)
    phase0 = draw(ds, 1, "rand", (1, H))
    sine = draw(ds, 2, "randn", (1, L, H))
    adain = [draw(ds, 3 + k, "randn", (1, C, Lk)) for k, (C, Lk) in enumerate(adain_shapes)]
    assert int(g["n_draws"]) == 3 + len(adain) and z_noise.shape[-1] == T
    return z_noise, phase0, sine, adain


def f0_upsampled(f0, upp, linear):
    """f0 [B][T] f32 -> [B][T*upp] f32 as the reference upsamples it (torch on the host)."""
    x = torch.from_numpy(np.ascontiguousarray(f0, np.float32))[:, None, :]
    if linear:
        y = torch.nn.functional.interpolate(x, size=x.shape[-1] * upp, mode="linear")
    else:
        y = torch.nn.Upsample(scale_factor=upp)(x)
    return y[:, 0].numpy()


def np_harmonic_source(f0, phase0, noise, upp, sr, lin_w, lin_b, linear):
    """SineGenerator + merge (mrf_hifigan.py:45-94, refinegan.py:66-107) restated in numpy float64: f0 [B][T], phase0
    [B][H] (harmonic 0's zero), noise [B][L][H] -> har [B][L] f64.  The per-sample increments are the reference's f32
    values; everything after them is float64 (the cumulative phase is exact to ~1e-12 cycles)."""
    f0u = f0_upsampled(f0, upp, linear)  # [B][L] f32
    B, L = f0u.shape
    H = len(lin_w)
    h = np.arange(1, H + 1, dtype=np.float32)
    rad = np.mod((f0u[:, :, None] * h[None, None, :]) / np.float32(sr), np.float32(1.0)).astype(np.float32)
    rad[:, 0, :] = rad[:, 0, :] + np.asarray(phase0, np.float32)
    cum = np.cumsum(rad.astype(np.float64), axis=1)
    sine = np.sin(2.0 * np.pi * (cum - np.floor(cum))) * 0.1
    uv = (f0u > 0).astype(np.float64)[:, :, None]
    waves = sine * uv + (uv * 0.003 + (1.0 - uv) * 0.1 / 3.0) * np.asarray(noise, np.float64)
    return np.tanh(waves @ np.asarray(lin_w, np.float64) + float(lin_b))


def rms(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(np.mean((a - b) ** 2)))
