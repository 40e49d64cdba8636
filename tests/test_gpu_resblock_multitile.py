"""Fused ResBlock pair (csrc/resblock.hip) where every workgroup walks more than one tile: with one persistent
workgroup per CU, tests/test_gpu_resblock.py's lengths (<= 39 tiles) never reach the weight ring running across a tile
seam, the R buffers reused by tile parity, the next-tile prefetch, or constants fetched once per block and used by a
later tile.  Here L = 2 nCU 240 + 37 (every block walks 2-3 tiles of 240 outputs, more of the narrow C = 64 form's 112)
and two clips of nCU 240 + 5 (tile numbering runs on across the clip seam), nCU read from the device."""
import functools

import pytest
import torch

from rvc_amd import ops
from test_gpu_resblock import DEV, make_pair, torch_ref, two_launch

pytestmark = pytest.mark.gpu

KD = [(3, 1), (11, 5)]
SHAPES = ["long", "two_clips"]


def shape(name):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return (1, 2 * ncu * 240 + 37) if name == "long" else (2, ncu * 240 + 5)


@functools.lru_cache(maxsize=None)
def case(C, K, d, name):
    """Weights, x, the accumulate operand (CPU) and the two convs, one per (C, K, d, shape) for every test."""
    B, L = shape(name)
    w, c1, c2 = make_pair(C, K, seed=C * 100 + K * 10 + d + B)
    g = torch.Generator().manual_seed(C + K + d + L)
    x = torch.randn(B, C, L, generator=g)
    acc0 = torch.randn(B, C, L, generator=g)
    return w, c1, c2, x, acc0


@functools.lru_cache(maxsize=None)
def cpu_ref(C, K, d, name):
    w, _, _, x, _ = case(C, K, d, name)
    return torch.stack([torch_ref(x[b], w, K, d) for b in range(x.shape[0])])


def fused(x, acc0, c1, c2, d):
    """The pair over [B][C][L] in one launch, plain (into NaNs) and accumulating."""
    B = x.shape[0]
    y = torch.full_like(x, float("nan"))
    ya = acc0.clone()
    ops.resblock_pair(x if B > 1 else x[0], y if B > 1 else y[0], c1, c2, d, 0.1)
    ops.resblock_pair(x if B > 1 else x[0], ya if B > 1 else ya[0], c1, c2, d, 0.1, accumulate=True)
    return y, ya


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K,d", KD)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32x6"])
def test_multitile_bit_identical_to_two_launches(precision, C, K, d, name):
    _, c1, c2, x, acc0 = case(C, K, d, name)
    x, acc0 = x.to(DEV), acc0.to(DEV)
    with ops.precision(precision), ops.splitk_target(0):
        assert ops.resblock_fusable(c1, c2, d)
        y, ya = fused(x, acc0, c1, c2, d)
        ref, refa = torch.empty_like(x), acc0.clone()
        for b in range(x.shape[0]):  # clip by clip: each clip of the batched launch equals its own call
            two_launch(x[b], c1, c2, K, d, y=ref[b])
            two_launch(x[b], c1, c2, K, d, y=refa[b], accumulate=True)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    assert torch.equal(y, ref)
    assert torch.equal(ya, refa)


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K,d", KD)
@pytest.mark.parametrize("C", [32, 64])
def test_multitile_f16x3(C, K, d, name):
    """Split-fp16 (the default path's kernels): within 2e-5 of the output's max of torch's fp32 pair on the CPU, the
    bound of test_fused_pair_f16x3."""
    _, c1, c2, x, acc0 = case(C, K, d, name)
    r = cpu_ref(C, K, d, name)
    with ops.precision("f16x3"):
        assert ops.resblock_fusable(c1, c2, d)
        y, ya = fused(x.to(DEV), acc0.to(DEV), c1, c2, d)
    torch.cuda.synchronize()
    y, ya = y.cpu(), ya.cpu()
    assert not torch.isnan(y).any() and not torch.isnan(ya).any()
    tol = 2e-5 * r.abs().max().item()
    err, erra = (y - r).abs().max().item(), (ya - (r + acc0)).abs().max().item()
    print(f"C {C} K {K} d {d} {name}: err {err:.3e} acc {erra:.3e} tol {tol:.3e}")
    assert err <= tol
    assert erra <= tol + 2e-6 * acc0.abs().max().item()


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K,d", KD)
def test_multitile_outputs_through_lds_bit_identical(K, d, name):
    """C = 32 split-fp16: the outputs stored by the compute waves (0), by the loader waves from R at the next tile's
    start (1) and from the other-parity R buffer after the next tile's S1 (2, the default) are the same bits."""
    C = 32
    _, c1, c2, x, acc0 = case(C, K, d, name)
    x, acc0 = x.to(DEV), acc0.to(DEV)
    lib = ops._lib.load()
    outs = []
    for on in (0, 1, 2):
        lib.rvc_resblock_set_ylds(on)
        try:
            with ops.precision("f16x3"):
                y, ya = fused(x, acc0, c1, c2, d)
            torch.cuda.synchronize()
            outs.append((y.cpu(), ya.cpu()))
        finally:
            lib.rvc_resblock_set_ylds(-1)
    assert not torch.isnan(outs[0][0]).any()
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and not torch.isnan(o[0]).any()
        assert torch.equal(outs[0][1], o[1])
