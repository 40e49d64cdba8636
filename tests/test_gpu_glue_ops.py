"""The small kernels of csrc/elementwise.hip and csrc/pipeline.hip, one op at a time, at the sizes where a last block, a
batch offset or a tie can go wrong: T = 1 and T around the 256-thread block, B > 1 with every clip different, the
pitchf == 1 tie of the protect blend, the peak exactly at 0.99, the counter-stream contract of the Philox draws.

References are torch / NumPy on the CPU, in f64 wherever an f32 CPU evaluation would not be bit-defined.  Bounds are
derived, not tuned: a value the device computes with n f32-rounded operations may differ from the f64 reference by
n * 2^-23 relative to the sum of the magnitudes of its terms (one ulp per rounding, twice the worst case); where the
operation is exact or one correctly rounded IEEE operation, the result is bit-equal."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rvc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_cell(cell, y, B):
    """cell (B cells) == max |y[b]| for every batch element, exactly (as tests/test_gpu_amax.py)."""
    y = y.reshape(B, -1)
    for b in range(B):
        want = float(y[b].abs().max().item())
        got = ops.amax_value(cell, b)
        assert got == want, (b, got, want)
        assert np.isfinite(got) and got > 0


def assert_within(got, ref, n, mag, what=""):
    """|got - ref| <= n * 2^-23 * mag elementwise (ref, mag f64)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert got.numel() > 0 and bool(torch.isfinite(got).all())
    over = (got - ref).abs() - n * ULP * mag
    assert float(over.max()) <= 0, (what, float(over.max()), float(((got - ref).abs() / mag.clamp_min(1e-300)).max()) / ULP)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------- textenc_embed
@pytest.mark.parametrize("with_emb", [True, False], ids=["emb", "noemb"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_textenc_embed(T, B, with_emb):
    """out = lrelu((lin + emb[pitch]) * scale, 0.1): add, multiply, multiply -- n = 3 roundings of (|lin| + |emb|) *
    scale (* slope on the negative side); the |max| cell exact per clip.  Every clip has its own pitches."""
    C = 192
    g = gen(10 * T + B)
    lin = torch.randn(B, C, T, generator=g)
    emb = torch.randn(256, C, generator=g)
    pitch = torch.randint(0, 256, (B, T), generator=g)
    pitch[0, 0], pitch[B - 1, T - 1] = 0, 255
    if T > 1:
        pitch[B - 1, 0] = 255
    scale, slope = float(np.float32(math.sqrt(C))), float(np.float32(0.1))
    e = emb[pitch].transpose(1, 2).double() if with_emb else torch.zeros(B, C, T, dtype=torch.float64)  # [B][C][T]
    pre = (lin.double() + e) * scale
    mag = (lin.double().abs() + e.abs()) * scale
    ref = torch.where(pre >= 0, pre, pre * slope)
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    # the slope shrinks the magnitude only where the sign is beyond doubt (|pre| above the sum's own rounding)
    mag = torch.where(pre < -4 * ULP * mag, mag * slope, mag)
    for amax in (False, True):
        out = torch.full((B, C, T), float("nan"), device=DEV)
        cells = ops.AmaxSlots(1, DEV, B) if amax else None
        ops.textenc_embed(lin.to(DEV), emb.to(DEV) if with_emb else None, pitch.to(DEV) if with_emb else None, out, B,
                          C, T, scale, slope, amax_out=cells[0] if amax else None)
        torch.cuda.synchronize()
        assert_within(out, ref, 3, mag, "textenc_embed")
        if amax:
            assert_cell(cells[0], out, B)


# ---------------------------------------------------------------- prior_sample
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 257])
def test_prior_sample(T, B):
    """zp = m + exp(logs) * noise * nscale, logs in [-6, 2]: expf counted as 2 roundings, two multiplies and the add
    -- n = 5 of |m| + |exp(logs) noise nscale|."""
    C = 192
    g = gen(20 * T + B)
    m = torch.randn(B, C, T, generator=g)
    logs = torch.rand(B, C, T, generator=g) * 8 - 6
    logs.view(-1)[0], logs.view(-1)[-1] = -6.0, 2.0
    noise = torch.randn(B, C, T, generator=g)
    nscale = float(np.float32(0.66666))
    stats = torch.cat([m, logs], 1).contiguous()  # [B][2C][T]
    term = torch.exp(logs.double()) * noise.double() * nscale
    zp = torch.full((B, C, T), float("nan"), device=DEV)
    ops.prior_sample(stats.to(DEV), noise.to(DEV), zp, B, C, T, nscale)
    torch.cuda.synchronize()
    assert_within(zp, m.double() + term, 5, m.double().abs() + term.abs(), "prior_sample")


# ---------------------------------------------------------------- gate, flip_channels, transpose with B > 1
def test_gate_batched():
    """tanh(a[c]) * sigmoid(a[c + H]), B = 2, H = 5, T = 257: tanhf (2 ulp = 2 roundings), expf (2), the add, the
    reciprocal and the product -- n = 7 of |out|."""
    B, H, T = 2, 5, 257
    a = torch.randn(B, 2 * H, T, generator=gen(30)) * 3
    out = torch.full((B, H, T), float("nan"), device=DEV)
    ops.gate(a.to(DEV), out, B, H, T)
    torch.cuda.synchronize()
    ad = a.double()
    ref = torch.tanh(ad[:, :H]) * torch.sigmoid(ad[:, H:])
    assert_within(out, ref, 7, ref.abs(), "gate")


def test_flip_channels_batched_odd():
    B, C, T = 2, 7, 257
    x = torch.randn(B, C, T, generator=gen(31))
    out = torch.full((B, C, T), float("nan"), device=DEV)
    ops.flip_channels(x.to(DEV), out, B, C, T)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(torch.flip(x, [1])))


@pytest.mark.parametrize("R,C", [(31, 33), (1, 100), (100, 1), (64, 64)])
def test_transpose_batched(R, C):
    B = 3
    x = torch.randn(B, R, C, generator=gen(R + C))
    out = torch.full((B, C, R), float("nan"), device=DEV)
    ops.transpose(x.to(DEV), out, B, R, C)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(x.transpose(1, 2)))


# ---------------------------------------------------------------- phone_upsample
PITCHF_EDGES = [0.0, float(np.nextafter(np.float32(1), np.float32(0))), 1.0,
                float(np.nextafter(np.float32(1), np.float32(2))), 200.0]


@pytest.mark.parametrize("mode", ["blend", "alias", "noblend"])
@pytest.mark.parametrize("C", [256, 768])
@pytest.mark.parametrize("Tf,T", [(50, 100), (50, 99), (1, 1), (1, 2), (129, 257)])
def test_phone_upsample(Tf, T, C, mode):
    """out[c][t] = f[c][t/2] p + f0[c][t/2] (1 - p), p = protect where pitchf[t] < 1 else 1.  pitchf walks 0, the
    largest f32 below 1, exactly 1, the next f32 above 1 and 200.  Where p == 1 the output is feats[t // 2] bit for
    bit; elsewhere, with (1 - p) taken as the device's own f32 difference, two products and the add -- n = 3 of
    |f p| + |f0 (1 - p)|.  alias: feats0 is feats.  noblend: pitchf = None."""
    g = gen(Tf + T + C)
    feats = torch.randn(C, Tf, generator=g)
    feats0 = torch.randn(C, Tf, generator=g)
    protect = 0.33
    pitchf = torch.tensor([PITCHF_EDGES[(t + 1) % 5] for t in range(T)], dtype=torch.float32)  # t = 0 blends
    if T >= 5:
        perm = torch.randperm(T, generator=g)
        pitchf = pitchf[perm]
    fd = feats.to(DEV)
    f0d = fd if mode == "alias" else feats0.to(DEV)
    out = torch.full((C, T), float("nan"), device=DEV)
    ops.phone_upsample(fd, None if mode == "noblend" else f0d, None if mode == "noblend" else pitchf.to(DEV), out, C,
                       Tf, T, protect)
    torch.cuda.synchronize()
    idx = torch.arange(T) // 2
    up = feats[:, idx]
    if mode == "noblend":
        assert torch.equal(bits(out), bits(up))
        return
    up0 = (feats if mode == "alias" else feats0)[:, idx]
    low = pitchf < 1.0  # the tie: exactly 1 is NOT below 1
    assert [bool(b) for b in (torch.tensor(PITCHF_EDGES, dtype=torch.float32) < 1.0)] == [True, True, False, False, False]
    p32 = np.float32(protect)
    p, omp = float(p32), float(np.float32(1) - p32)
    got = out.cpu()
    assert torch.equal(bits(got[:, ~low]), bits(up[:, ~low]))
    a, b = up[:, low].double() * p, up0[:, low].double() * omp
    assert_within(got[:, low], a + b, 3, a.abs() + b.abs(), "phone_upsample")


# ---------------------------------------------------------------- peak_normalize
PEAK_N = [1, 255, 257, 2048 * 256 + 77]  # the last: the grid-stride loop takes a second trip


def _peak_run(x, ws=None):
    ws = torch.full((4,), 0x7F7F7F7F, dtype=torch.int32, device=DEV) if ws is None else ws  # (the op clears it)
    xd = x.to(DEV)
    so = torch.full((1,), float("nan"), device=DEV)
    ops.peak_normalize(xd, ws, so)
    torch.cuda.synchronize()
    return xd.cpu(), np.float32(so.cpu().numpy()[0]), ws


def _quiet(n, seed):
    return (torch.rand(n, generator=gen(seed)) - 0.5) * 0.8  # |x| < 0.4


@pytest.mark.parametrize("n", PEAK_N)
def test_peak_normalize(n):
    """m = max |x| / 0.99 in f32; x /= m only if m > 1 -- a true (correctly rounded) division."""
    f99 = np.float32(0.99)
    # peak 0.5: unchanged, scale_out = f32(0.5) / f32(0.99)
    x = _quiet(n, n)
    x[n // 2] = -0.5
    got, so, _ = _peak_run(x)
    assert torch.equal(bits(got), bits(x)) and so == np.float32(0.5) / f99
    # peak exactly f32(0.99): m == 1 exactly, unchanged
    x = _quiet(n, n + 1)
    x[0] = float(f99)
    got, so, _ = _peak_run(x)
    assert so == np.float32(1.0) and torch.equal(bits(got), bits(x))
    # peak -3 in the last element: every element is NumPy's f32 x / m
    x = _quiet(n, n + 2)
    x[n - 1] = -3.0
    got, so, _ = _peak_run(x)
    m = np.float32(3.0) / f99
    assert so == m and m > 1
    assert np.array_equal((x.numpy() / m).view(np.int32), got.numpy().view(np.int32))
    # all zeros
    got, so, _ = _peak_run(torch.zeros(n))
    assert so == np.float32(0.0) and torch.equal(bits(got), bits(torch.zeros(n)))


def test_peak_normalize_workspace_reuse():
    """Two calls on one workspace, the larger peak first: the second must not see the first's maximum."""
    n = 1000
    x1 = _quiet(n, 1)
    x1[7] = 3.0
    _, so1, ws = _peak_run(x1)
    assert so1 == np.float32(3.0) / np.float32(0.99)
    x2 = _quiet(n, 2)
    x2[n - 1] = 0.5
    got, so2, _ = _peak_run(x2, ws)
    assert so2 == np.float32(0.5) / np.float32(0.99) and torch.equal(bits(got), bits(x2))


# ---------------------------------------------------------------- rms_frames, rms_mix, change_rms
def dev_rms_frames(src, hop):
    """rvc_rms_frames of a device f64 or f32 signal -> [1 + n / hop] on the CPU."""
    lib = ops._lib.load()
    n = src.numel()
    nf = lib.rvc_rms_frames_len(n, hop)
    assert nf == 1 + n // hop
    out = torch.full((nf + 2,), -7.0, device=DEV)
    p = ctypes.c_void_p(src.data_ptr())
    is64 = src.dtype == torch.float64
    ops.check(lib.rvc_rms_frames(p if is64 else None, None if is64 else p, n, hop, ops._p(out), ops._stream()),
              "rms_frames")
    torch.cuda.synchronize()
    out = out.cpu()
    assert float(out[nf]) == -7.0 and float(out[nf + 1]) == -7.0  # nothing past the last frame
    return out[:nf]


def np_rms_frames(y, hop):
    """librosa.feature.rms(y, frame_length=2 hop, hop_length=hop) restated: zero-pad by hop, frames of 2 hop at stride
    hop, f32 squares, f64 mean, f32 sqrt."""
    y32 = np.asarray(y).astype(np.float32)
    sq = np.pad(y32 * y32, hop).astype(np.float64)
    nf = 1 + y32.size // hop
    mean = np.array([sq[f * hop:f * hop + 2 * hop].sum() / (2 * hop) for f in range(nf)])
    return np.sqrt(mean.astype(np.float32))


def rms_sizes(hop):
    return [hop - 1, hop, 2 * hop + 1, 5 * hop + hop // 2]


def signal(n, seed, dtype):
    t = torch.randn(n, generator=gen(seed), dtype=torch.float64) * 0.3
    return t if dtype == "f64" else t.float()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hop,n", [(64, n) for n in rms_sizes(64)] + [(8000, 8000 * 2 + 1)])
def test_rms_frames(hop, n, dtype):
    """Against the NumPy restatement: the f64 sum's order is far below f32, leaving the mean's rounding to f32 and the
    square root -- n = 2."""
    y = signal(n, n + hop, dtype)
    if n > 3 * hop:
        y[hop:3 * hop] = 0  # frame 2 is silent
    got = dev_rms_frames(y.to(DEV), hop)
    ref = torch.from_numpy(np_rms_frames(y.numpy(), hop)).double()
    if n > 3 * hop:
        assert float(got[2]) == 0.0
    assert_within(got, ref, 2, ref.abs(), "rms_frames")


def torch_rms_mix(y, r1, r2, rate):
    """convert.py:150-152 on the CPU in f32: both envelopes to the output length by F.interpolate(linear), then
    y * r1^(1 - rate) * max(r2, 1e-6)^(rate - 1)."""
    n = y.numel()
    a = F.interpolate(r1.view(1, 1, -1), size=n, mode="linear").view(-1)
    b = F.interpolate(r2.view(1, 1, -1), size=n, mode="linear").view(-1)
    return y * (torch.pow(a, 1 - rate) * torch.pow(torch.maximum(b, torch.zeros_like(b) + 1e-6), rate - 1))


@pytest.mark.parametrize("rate", [0.0, 0.35, 1.0])
@pytest.mark.parametrize("n,n1,n2", [(777, 5, 13), (777, 40, 13), (1, 1, 1), (257, 1, 5), (256, 300, 2),
                                     (16001, 3, 4)])
def test_rms_mix(n, n1, n2, rate):
    """n1 != n2, the source envelope shorter and longer than the output's; a silent output frame (the clamp to 1e-6)
    and a zero source frame.  test_change_rms_matches_reference's bound: rtol 2e-6, atol 1e-7.  rate = 1: both
    exponents are 0 and y is bit-unchanged.

    Next to a zero frame the interpolation weight 1 - l1 is small, so the result there follows the rounding of the
    source index: torch's CPU kernel fuses scale * (i + 0.5) - 0.5 and the blend (FMA), and so does the device.  With
    the index rounded twice these cases miss the bound by up to 1.5e-5 relative at n = 777 and 3e-4 at n = 16001 (two
    seconds of a clip at the real hop of 8000), which is how this test found it."""
    g = gen(n + n1 + n2)
    y = torch.randn(n, generator=g) * 0.2
    r1 = torch.rand(n1, generator=g) * 0.3 + 0.01
    r2 = torch.rand(n2, generator=g) * 0.3 + 0.01
    if n1 > 2:
        r1[n1 // 2] = 0.0
    if n2 > 2:
        r2[1] = 0.0
    yd = torch.cat([y, torch.full((3,), -7.0)]).to(DEV)
    r1d, r2d = r1.to(DEV), r2.to(DEV)
    ops.check(ops._lib.load().rvc_rms_mix(ops._p(yd), n, ops._p(r1d), n1, ops._p(r2d), n2, float(rate),
                                          ops._stream()), "rms_mix")
    torch.cuda.synchronize()
    got = yd.cpu()
    assert bool((got[n:] == -7.0).all())
    if rate == 1.0:
        assert torch.equal(bits(got[:n]), bits(y))
    np.testing.assert_allclose(got[:n].numpy(), torch_rms_mix(y, r1, r2, rate).numpy(), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hop,n_src,n_out", [(64, n, m) for n, m in zip(rms_sizes(64), reversed(rms_sizes(64)))]
                         + [(8000, 8000 * 2 + 1, 8000 * 3 - 5)])
def test_change_rms_chain(hop, n_src, n_out, dtype):
    """ops.change_rms (both envelopes + the mix) with the source shorter and longer than the output, against the NumPy
    envelopes mixed by torch on the CPU, within test_change_rms_matches_reference's bound."""
    src = signal(n_src, n_src, dtype)
    y = signal(n_out, n_out + 1, "f32")
    out = y.to(DEV)
    sd = src.to(DEV)
    ops.change_rms(sd if dtype == "f32" else None, sd if dtype == "f64" else None, out, hop, 0.35)
    torch.cuda.synchronize()
    r1 = torch.from_numpy(np_rms_frames(src.numpy(), hop))
    r2 = torch.from_numpy(np_rms_frames(y.numpy(), hop))
    np.testing.assert_allclose(out.cpu().numpy(), torch_rms_mix(y, r1, r2, 0.35).numpy(), rtol=2e-6, atol=1e-7)


# ---------------------------------------------------------------- the Philox counter stream
LO, HI = -0.25, 1.5
KINDS = {
    "randn": lambda out, seed, off: ops.randn(out, seed, off),
    "uniform": lambda out, seed, off: ops.rand_uniform(out, seed, off),
    "triang": lambda out, seed, off: ops.rand_triang(out, LO, HI, seed, off),
}


def draw(kind, n, seed, off=0):
    out = torch.full((n + 4,), -7.0, device=DEV)
    KINDS[kind](out[:n], seed, off)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[n:] == -7.0).all())  # a ragged last group of 4 stores only its own values
    return out[:n]


@pytest.mark.parametrize("kind", list(KINDS))
def test_counter_stream_offset(kind):
    """Value e of a call is draw e % 4 of counter e / 4 + offset: n values at offset k are elements [4k, 4k + n) of a
    call of n + 4k values at offset 0, bit for bit."""
    seed = 0x1234_5678_9ABC
    for k in (1, 7):
        for n in (1, 2, 3, 5, 1021):
            part = draw(kind, n, seed, k)
            whole = draw(kind, n + 4 * k, seed, 0)
            assert torch.equal(bits(part), bits(whole[4 * k:4 * k + n])), (kind, n, k)
    assert not torch.equal(draw(kind, 64, seed), draw(kind, 64, seed + 1))


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_seed_is_added(kind):
    """seed_add (ops.device_seed): the draws of seed s under a device seed a are those of the host-side sum s + a."""
    s, a = 77, (1 << 33) + 5
    with ops.device_seed(torch.tensor([a], dtype=torch.int64, device=DEV)):
        got = draw(kind, 1021, s)
    assert torch.equal(bits(got), bits(draw(kind, 1021, s + a)))
    assert not torch.equal(bits(got), bits(draw(kind, 1021, s)))


@pytest.mark.parametrize("kind", list(KINDS))
def test_draw_ranges_and_moments(kind):
    """Ranges, and the mean and variance over N = 2^20 draws within 5 standard errors, from the distribution's own
    moments: se(mean) = sqrt(var / N), se(variance) = sqrt((mu4 - var^2) / N)."""
    N = 1 << 20
    x = draw(kind, N, 4242).double()
    w = HI - LO
    mean, var, mu4 = {"randn": (0.0, 1.0, 3.0), "uniform": (0.5, 1 / 12, 1 / 80),
                      "triang": ((LO + HI) / 2, w * w / 24, w ** 4 / 240)}[kind]
    if kind == "uniform":
        assert float(x.min()) >= 0.0 and float(x.max()) < 1.0
    elif kind == "triang":
        assert float(x.min()) >= LO and float(x.max()) <= HI
    assert bool(torch.isfinite(x).all())
    assert abs(float(x.mean()) - mean) <= 5 * math.sqrt(var / N)
    assert abs(float(x.var(unbiased=False)) - var) <= 5 * math.sqrt((mu4 - var * var) / N)
