"""RMVPE's image glue (rmvpe.hip: mel_image, avgpool2, interleave4, img_to_seq) op by op, in f32 and f64, for one
image and for two taken from views with a batch stride larger than the image.  Every output is filled with NaN
before the launch, so a border cell the kernel leaves unwritten shows; interior, border rows, border columns and
corners are asserted apart.  The ops only move values (avgpool2 adds four in a fixed order and divides by 4), so
the results are exact -- except mel_image's product-sum, see its test."""
import pytest
import torch

from rvc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]


def rand(*shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).to(DEV)


def batched(B, *shape, dtype, fill=None, seed=0):
    """[(B)]shape: one tensor for B = 1, else a [:, :shape[0]] view of a buffer one channel (row) wider, so that the
    batch stride is larger than the image."""
    if B == 1:
        return rand(*shape, dtype=dtype, seed=seed) if fill is None else \
            torch.full(shape, fill, dtype=dtype, device=DEV)
    wide = (B, shape[0] + 1) + tuple(shape[1:])
    buf = rand(*wide, dtype=dtype, seed=seed) if fill is None else torch.full(wide, fill, dtype=dtype, device=DEV)
    return buf[:, :shape[0]]


def assert_bordered(got, want_interior, what):
    """got [...][H+2][W+2] against the interior [...][H][W] and a zero border, one cell class at a time."""
    assert got.shape[:-2] == want_interior.shape[:-2], what
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    assert torch.equal(got[..., 1:-1, 1:-1], want_interior), f"{what}: interior"
    assert torch.equal(got[..., 0, 1:-1], zero.expand_as(got[..., 0, 1:-1])), f"{what}: top border row"
    assert torch.equal(got[..., -1, 1:-1], zero.expand_as(got[..., -1, 1:-1])), f"{what}: bottom border row"
    assert torch.equal(got[..., 1:-1, 0], zero.expand_as(got[..., 1:-1, 0])), f"{what}: left border column"
    assert torch.equal(got[..., 1:-1, -1], zero.expand_as(got[..., 1:-1, -1])), f"{what}: right border column"
    corners = got[..., [0, 0, -1, -1], [0, -1, 0, -1]]
    assert torch.equal(corners, zero.expand_as(corners)), f"{what}: corners"


# (2, 2): the pooled plane has one interior cell, first and last in both directions (the deepest pooling of a clip
# of at most 32 frames); (2, 8) / (6, 4): one interior row / several; (34, 20): more than one 256-thread block
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(2, 2), (2, 8), (6, 4), (34, 20)])
def test_avgpool2(dtype, B, H, W):
    C = 3
    x = batched(B, C, H + 2, W + 2, dtype=dtype, seed=H * W)
    out = batched(B, C, H // 2 + 2, W // 2 + 2, dtype=dtype, fill=float("nan"))
    ops.avgpool2(x, out, C, H, W)
    i = x[..., 1:-1, 1:-1]
    want = (((i[..., 0::2, 0::2] + i[..., 0::2, 1::2]) + i[..., 1::2, 0::2]) + i[..., 1::2, 1::2]) / 4
    assert_bordered(out, want, f"avgpool2 {dtype} B={B} {H}x{W}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (9, 8)])
def test_interleave4(dtype, B, H, W):
    """The first C channels of a 2C-channel concat buffer are written (border included), the others left alone."""
    C = 2
    ph = batched(B, 4, C, H + 2, W + 2, dtype=dtype, seed=H * W)
    out = batched(B, 2 * C, 2 * H + 2, 2 * W + 2, dtype=dtype, fill=float("nan"))
    ops.interleave4(ph, out, C, H, W)
    want = torch.empty(*out.shape[:-3], C, 2 * H, 2 * W, dtype=dtype, device=DEV)
    for py in (0, 1):
        for px in (0, 1):
            want[..., py::2, px::2] = ph[..., py * 2 + px, :, 1:-1, 1:-1]
    assert_bordered(out[..., :C, :, :], want, f"interleave4 {dtype} B={B} {H}x{W}")
    assert torch.isnan(out[..., C:, :, :]).all(), "interleave4: wrote past its C channels"


# H = 300 crosses the 256-thread block
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 4), (300, 4)])
def test_img_to_seq(dtype, B, H, W):
    C = 3
    img = batched(B, C, H + 2, W + 2, dtype=dtype, seed=H)
    seq = batched(B, C * W, H, dtype=dtype, fill=float("nan"))
    ops.img_to_seq(img, seq, C, H, W)
    want = img[..., 1:-1, 1:-1].transpose(-1, -2).reshape(*img.shape[:-3], C * W, H)  # [c][t][f] -> [c*W + f][t]
    assert torch.equal(seq, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("M,F,Tp", [(5, 5, 8), (128, 33, 64)])
def test_mel_image(dtype, B, M, F, Tp):
    """img[t + 1][m + 1] = mel[m][reflect(t)] * scale + shift.  The kernel's product-sum may contract to an fma (one
    rounding) where torch rounds twice, so the interior is allowed 1 ulp: mel, scale and shift are all positive
    here, so the result is at least as large as the product and the product's rounding, half an ulp of the
    product, stays below one ulp of the result.  The border is exact."""
    scale, shift = 0.7310585786300049, 0.30000001192092896
    mel = batched(B, M, F, dtype=dtype, seed=M).abs() + 0.5
    mel = mel if B == 1 else torch.cat([mel, mel[:, :1]], 1)[:, :M]  # a strided view again after abs()
    img = batched(B, 1, Tp + 2, M + 2, dtype=dtype, fill=float("nan"))
    ops.mel_image(mel, img, M, F, Tp, scale, shift)
    src = torch.tensor([t if t < F else 2 * (F - 1) - t for t in range(Tp)], device=DEV)
    s, h = torch.tensor(scale, dtype=dtype, device=DEV), torch.tensor(shift, dtype=dtype, device=DEV)
    want = (mel[..., src] * s + h).transpose(-1, -2).unsqueeze(-3)  # [(B)][1][Tp][M]
    got = img[..., 1:-1, 1:-1]
    lo = torch.nextafter(want, torch.full_like(want, -float("inf")))
    hi = torch.nextafter(want, torch.full_like(want, float("inf")))
    assert bool(((got >= lo) & (got <= hi)).all()), f"mel_image {dtype} B={B}: interior"
    assert_bordered(img, got, f"mel_image {dtype} B={B} M={M} F={F} Tp={Tp}")
