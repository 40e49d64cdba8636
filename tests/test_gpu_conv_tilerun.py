"""The x6 conv engine's epilogues on the two tiles and store forms that tests/test_gpu_conv_x6_rows.py leaves out,
against torch's f64 conv on the CPU.

Column-tile runs (a block walking several column tiles) are not built, so nothing here varies the
tiles per block: these are the cases that stand without them, each one block per tile as every launch is today.

  * The 128 x 128 tile on 8 compute waves at C = 256 -> 256, B = 2, L = 3 x 128 + 5 (three full column tiles and a
    ragged one, two row tiles), (K, d) in {(3, 1), (11, 5)}, split-fp16 and 6-pass fp32x6, with a leaky-ReLU
    pre-activation, bias, a residual, and either a NaN-filled output or an accumulate run into a cloned operand with a
    second bias.  plan() would give split-fp16 the 256-wide tile at this size, so ONE child process runs every case
    under RVC_X6_BN256=0 (read once per process) and asserts the tile it got (ops.last_conv_tile()).
  * One polyphase ConvT launch (u = 4 phases, 2 taps each, C = 128 -> 128, B = 2) on the 128 x 256 tile, tile asserted:
    the row-base epilogue's strided stores (out_pos with ostride and phase), two column tiles per phase with a ragged
    last one, in both register layouts, which must give the same bits.

Every output must have no NaN left, a |max| cell equal to max |y| per batch element, and per output row an rms error
below 2^-18 of the rms of the row's sum of |products| -- test_gpu_ops.py::test_conv1d_f16x3's bound for split-fp16; the
6-pass arithmetic (24-bit operands in three bf16 parts, the same f32 accumulation) is held to the same bound.  Measured
on an MI355X: 3.2e-8 to 5.8e-8 in every case, against the 3.8e-6 allowed."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, B, L = 256, 2, 3 * 128 + 5
BOUND = 2.0 ** -18

# name: K, d, prec, epilogue ("rb": residual into a NaN-filled output; "full": + bias2, accumulate into a clone)
CASES = {f"k{K}_{prec}_{epi}": (K, d, prec, epi)
         for K, d in ((3, 1), (11, 5)) for prec in ("f16x3", "fp32x6") for epi in ("rb", "full")}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def inputs(name):
    K = CASES[name][0]
    g = gen(sum(map(ord, name)))
    return dict(x=torch.randn(B, C, L, generator=g), w=torch.randn(C, C, K, generator=g) / math.sqrt(C * K),
                b=torch.randn(C, generator=g) * 0.1, b2=torch.randn(C, generator=g) * 0.1,
                res=torch.randn(B, C, L, generator=g), acc0=torch.randn(B, C, L, generator=g))


def run_case(ops, name):
    """-> (y [B][C][L] on the CPU, the cell's |max| per batch element); the 128 x 128 tile, asserted."""
    K, d, prec, epi = CASES[name]
    t = inputs(name)
    c = ops.Conv(t["w"], t["b"])
    y = t["acc0"].to(DEV) if epi == "full" else torch.full((B, C, L), float("nan"), device=DEV)
    kw = dict(pad=d * (K - 1) // 2, dil=d, out=y, res=t["res"].to(DEV), in_act=ops.ACT_LRELU, in_slope=0.1)
    if epi == "full":
        kw.update(bias2=t["b2"].to(DEV), accumulate=True)
    cells = ops.AmaxSlots(1, DEV, B)
    with ops.precision(prec), ops.splitk_target(0):
        c(t["x"].to(DEV), amax_out=cells[0], **kw)
    assert ops.LAST_CONV_ENGINE == 1 and ops.LAST_CONV_WS == 0
    assert ops.last_conv_tile() == (128, 128), (name, ops.last_conv_tile())
    torch.cuda.synchronize()
    return y.cpu(), [ops.amax_value(cells[0], b) for b in range(B)]


def row_error(y, ref, mag):
    """Worst output row's rms error over the rms of its sum of |products| ([B][Co][L] tensors)."""
    Co = y.shape[1]
    err = (y.double() - ref).transpose(0, 1).reshape(Co, -1)
    return float((err.pow(2).mean(1).sqrt() / mag.transpose(0, 1).reshape(Co, -1).pow(2).mean(1).sqrt()).max())


@pytest.fixture(scope="module")
def ops():
    from rvc_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture(scope="module")
def narrow(tmp_path_factory):
    """Every case on the 128 x 128 tile: this file as a script in one child process under RVC_X6_BN256=0."""
    out = tmp_path_factory.mktemp("x6_tiles") / "narrow.npz"
    env = dict(os.environ, RVC_X6_BN256="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", list(CASES))
def test_tile128_c256_against_f64(narrow, name):
    K, d, prec, epi = CASES[name]
    t = inputs(name)
    xa = F.leaky_relu(t["x"].double(), 0.1)
    bias = t["b"].double() + (t["b2"].double() if epi == "full" else 0)
    ref = F.conv1d(xa, t["w"].double(), bias, 1, d * (K - 1) // 2, d) + t["res"].double()
    mag = F.conv1d(xa.abs(), t["w"].double().abs(), bias.abs(), 1, d * (K - 1) // 2, d)
    if epi == "full":
        ref = ref + t["acc0"].double()
    y = torch.from_numpy(narrow[name])
    assert not torch.isnan(y).any()
    for b in range(B):
        assert float(narrow[name + "__amax"][b]) == float(y[b].abs().max()), (b, narrow[name + "__amax"][b])
    rel = row_error(y, ref, mag)
    print(name, "worst row: rms error / rms sum of |products| =", rel, "bound", BOUND)
    assert rel < BOUND, rel


def test_polyphase_convt_wide_tile(ops):
    Ci, Co, u, K, Lin = 128, 128, 4, 8, 256 + 91
    p = (K - u) // 2
    g = gen(41)
    x = torch.randn(B, Ci, Lin, generator=g)
    w = torch.randn(Ci, Co, K, generator=g) / math.sqrt(Ci * K / u)
    b = torch.randn(Co, generator=g) * 0.1
    up = ops.ConvT(w, b, u, p)
    Lout = up.out_len(Lin)
    lib = ops._lib.load()
    ys = []
    for swz in (1, 0):
        y = torch.full((B, Co, Lout), float("nan"), device=DEV)
        cells = ops.AmaxSlots(1, DEV, B)
        lib.rvc_conv1d_set_swz(swz)
        try:
            with ops.precision("f16x3"), ops.splitk_target(0):
                up(x.to(DEV), out=y, in_act=ops.ACT_LRELU, in_slope=0.1, amax_out=cells[0])
        finally:
            lib.rvc_conv1d_set_swz(-1)
        assert ops.LAST_CONV_ENGINE == 1 and ops.LAST_CONV_PASSES == ops.F16X3 and ops.LAST_CONV_WS == 0
        assert ops.last_conv_tile() == (128, 256), ops.last_conv_tile()
        torch.cuda.synchronize()
        y = y.cpu()
        assert not torch.isnan(y).any()
        for i in range(B):
            assert ops.amax_value(cells[0], i) == float(y[i].abs().max()), i
        ys.append(y)
    assert torch.equal(ys[0], ys[1]), (ys[0] - ys[1]).abs().max()
    xa = F.leaky_relu(x.double(), 0.1)
    ref = F.conv_transpose1d(xa, w.double(), b.double(), u, p)
    mag = F.conv_transpose1d(xa.abs(), w.double().abs(), b.double().abs(), u, p)
    rel = row_error(ys[0], ref, mag)
    print("ConvT u = 4: worst row: rms error / rms sum of |products| =", rel, "bound", BOUND)
    assert rel < BOUND, rel


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "rvc-maker_amd"))
    from rvc_amd import ops as _ops
    _ops._lib.load()
    res = {}
    for n in CASES:
        yy, mm = run_case(_ops, n)
        res[n], res[n + "__amax"] = yy.numpy(), np.array(mm, dtype=np.float64)
    np.savez(sys.argv[1], **res)
