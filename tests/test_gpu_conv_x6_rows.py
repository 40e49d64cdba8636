"""The 256-wide x6 tile's row-base epilogue (csrc/conv1d.hip conv_epilogue_rows) and the epilogue constants in LDS
(epi_bias), for the ResBlock convs of the C = 128 generator stage (main/library/algorithm/residuals.py:36-44).

Every split-fp16 case with Co % 16 == 0 runs the 128 x 256 tile in this process -- asserted per launch from the tile
plan() chose (ops.last_conv_tile()), as is the 128 x 128 tile in the child process below, so that no comparison can
quietly run one tile against itself -- in both register layouts (rvc_conv1d_set_swz 1 / 0), with outputs written
into NaN-filled (or cloned accumulate) buffers, and must give

  * the same bits in both layouts, no NaN left, and a |max| cell equal to max |y| per batch element;
  * the same bits as the 128 x 128 tile -- the per-element epilogue this one replaces on the wide tile, with the
    unrolled activations -- computed by ONE child process under RVC_X6_BN256=0 (plan() reads that switch once per
    process; the k order per element does not depend on the tile, so the sums are the same bits);
  * for the cases without an output activation, torch's f64 conv on the CPU within test_conv1d_f16x3's bound (per
    output row, rms error below 2^-18 of the rms of the row's sum of |products|), so that "same bits" is not relative
    to a broken baseline.

Shapes: L = 5 x 256 + 37 gives six column tiles with a ragged last one (the masked stores) and five full ones (the
straight-line stores); B = 2; Co = 192 and 144 leave the second row tile with 4 and 1 of its 8 row fragments (the
skipped fragments); Co = 136 is no multiple of 16 and must run 128 wide, and so must the 6-pass fp32x6 case (the wide
tile is split-fp16's): those two pin the constants' LDS table on the narrow tile; tanh / GELU take the rolled
activation loop; the default split-K target splits the 128-channel conv in two (the partial tiles' stores).  Every
case has at most 22 tiles 128 wide and at least 4 fewer 256 wide: on a device of 256 CUs both grids are a fraction of
one round and their fill differs by less than plan()'s 0.05, so it picks the wide tile; on a device where it would
not, the tile assertion fails instead of the comparison passing for nothing."""
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
L6 = 5 * 256 + 37

# name: Ci, Co, K, d, L, B, prec, epilogue, output activation, split-K
CASES = {
    "rb_k3": (128, 128, 3, 1, L6, 2, "f16x3", "rb", "none", False),
    "rb_k11": (128, 128, 11, 5, L6, 2, "f16x3", "rb", "none", False),
    "full_k3": (128, 128, 3, 1, L6, 2, "f16x3", "full", "none", False),
    "full_k11": (128, 128, 11, 5, L6, 2, "f16x3", "full", "none", False),
    "full_k3_fp32x6": (128, 128, 3, 1, L6, 2, "fp32x6", "full", "none", False),
    "full_tanh": (128, 128, 3, 1, 2 * 256 + 5, 1, "f16x3", "full", "tanh", False),
    "rb_gelu_co192": (128, 192, 1, 1, 256 + 91, 2, "f16x3", "rb", "gelu", False),
    "rb_co144": (128, 144, 3, 1, 256 + 91, 1, "f16x3", "rb", "none", False),
    "rb_co136": (128, 136, 3, 1, 256 + 91, 1, "f16x3", "rb", "none", False),
    "full_splitk": (128, 128, 3, 1, L6, 2, "f16x3", "full", "none", True),
    "plain_splitk_co192": (128, 192, 7, 1, 256 + 91, 1, "f16x3", "plain", "none", True),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def inputs(name):
    Ci, Co, K, d, L, B = CASES[name][:6]
    g = gen(sum(map(ord, name)))
    return dict(x=torch.randn(B, Ci, L, generator=g), w=torch.randn(Co, Ci, K, generator=g) / math.sqrt(Ci * K),
                b=torch.randn(Co, generator=g) * 0.1, b2=torch.randn(Co, generator=g) * 0.1,
                res=torch.randn(B, Co, L, generator=g), acc0=torch.randn(B, Co, L, generator=g))


def want_tile(name):
    """The (rows, columns) tile a case must run on: 128 x 256 for split-fp16 with Co % 16 == 0, unless switched off."""
    wide = CASES[name][6] == "f16x3" and CASES[name][1] % 16 == 0 and os.environ.get("RVC_X6_BN256") != "0"
    return (128, 256) if wide else (128, 128)


def run_case(ops, name, swz=-1):
    """-> (y [B][Co][L] on the CPU, the cell's |max| per batch element)."""
    Ci, Co, K, d, L, B, prec, epi, act, split = CASES[name]
    t = inputs(name)
    c = ops.Conv(t["w"], t["b"])
    y = t["acc0"].to(DEV) if epi == "full" else torch.full((B, Co, L), float("nan"), device=DEV)
    kw = dict(pad=d * (K - 1) // 2, dil=d, out=y if B > 1 else y[0], in_act=ops.ACT_LRELU, in_slope=0.1)
    if epi != "plain":
        kw.update(res=t["res"].to(DEV) if B > 1 else t["res"][0].to(DEV))
    if epi == "full":
        kw.update(bias2=t["b2"].to(DEV), accumulate=True)
    if act != "none":
        kw.update(out_act=ops.ACT_TANH if act == "tanh" else ops.ACT_GELU, out_scale=-1.5)
    cells = ops.AmaxSlots(1, DEV, B)
    lib = ops._lib.load()
    lib.rvc_conv1d_set_swz(swz)
    try:
        with ops.precision(prec):
            if split:
                c(t["x"].to(DEV) if B > 1 else t["x"][0].to(DEV), amax_out=cells[0], **kw)
                assert ops.LAST_CONV_WS > 0
            else:
                with ops.splitk_target(0):
                    c(t["x"].to(DEV) if B > 1 else t["x"][0].to(DEV), amax_out=cells[0], **kw)
                assert ops.LAST_CONV_WS == 0
        assert ops.LAST_CONV_ENGINE == 1
        assert ops.last_conv_tile() == want_tile(name), (name, ops.last_conv_tile())
    finally:
        lib.rvc_conv1d_set_swz(-1)
    torch.cuda.synchronize()
    return y.cpu(), [ops.amax_value(cells[0], b) for b in range(B)]


@pytest.fixture(scope="module")
def ops():
    from rvc_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture(scope="module")
def narrow(tmp_path_factory):
    """Every case on the 128 x 128 tile: this file as a script in one child process under RVC_X6_BN256=0."""
    out = tmp_path_factory.mktemp("x6_rows") / "narrow.npz"
    env = dict(os.environ, RVC_X6_BN256="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", list(CASES))
def test_rows_epilogue_same_bits(ops, narrow, name):
    B = CASES[name][5]
    y1, m1 = run_case(ops, name, swz=1)
    y0, m0 = run_case(ops, name, swz=0)
    assert not torch.isnan(y1).any() and not torch.isnan(y0).any()
    assert torch.equal(y1, y0), (y1 - y0).abs().max()
    want = torch.from_numpy(narrow[name])
    assert torch.equal(y1, want), (y1 - want).abs().max()
    for b in range(B):
        peak = float(y1[b].abs().max())
        assert m1[b] == peak and m0[b] == peak, (b, m1[b], m0[b], peak)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[8] == "none" and c[6] == "f16x3"])
def test_rows_epilogue_against_f64(ops, name):
    Ci, Co, K, d, L, B, prec, epi, act, split = CASES[name]
    t = inputs(name)
    xa = F.leaky_relu(t["x"].double(), 0.1)
    bias = t["b"].double() + (t["b2"].double() if epi == "full" else 0)
    ref = F.conv1d(xa, t["w"].double(), bias, 1, d * (K - 1) // 2, d)
    mag = F.conv1d(xa.abs(), t["w"].double().abs(), bias.abs(), 1, d * (K - 1) // 2, d)
    if epi != "plain":
        ref = ref + t["res"].double()
    if epi == "full":
        ref = ref + t["acc0"].double()
    y, _ = run_case(ops, name)
    err = (y.double() - ref).transpose(0, 1).reshape(Co, -1)
    rel = err.pow(2).mean(1).sqrt() / mag.transpose(0, 1).reshape(Co, -1).pow(2).mean(1).sqrt()
    print(name, "worst row: rms error / rms sum of |products| =", float(rel.max()), "bound", 2.0 ** -18)
    assert float(rel.max()) < 2.0 ** -18, float(rel.max())


@pytest.mark.parametrize("split", [False, True])
def test_rows_epilogue_2d_border(ops, split):
    """The wide tile in 2-D mode (a 3x3 conv on a zero-bordered [C][H+2][W+2] image, 9 tap offsets, three column tiles):
    the border cells are written as exactly 0 by the epilogue's border pass (split: by the split-K reduce, after the
    partial tiles' stores), nothing stays NaN, and the interior matches torch's f64 conv2d within split-fp16's error
    (2^-18 of the largest sum of |products|, the row bound of test_conv1d_f16x3 taken over the image)."""
    from rvc_amd.rmvpe import _Conv2d
    Ci, Co, H, W = 128, 128, 30, 20
    g = gen(3)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    b = torch.randn(Co, generator=g) * 0.1
    x = torch.randn(Ci, H, W, generator=g)
    conv = _Conv2d(w, b, DEV, f64=False)
    out = torch.full((Co, H + 2, W + 2), float("nan"), device=DEV)
    with ops.precision("f16x3"), ops.splitk_target(None if split else 0):
        conv(F.pad(x, (1, 1, 1, 1)).to(DEV).contiguous(), H, W, out)
    assert ops.LAST_CONV_ENGINE == 1 and ops.LAST_CONV_PASSES == ops.F16X3 and (ops.LAST_CONV_WS > 0) == split
    torch.cuda.synchronize()
    o = out.cpu()
    assert not torch.isnan(o).any()
    border = torch.ones(H + 2, W + 2, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert torch.equal(o[:, border], torch.zeros(Co, int(border.sum())))
    ref = F.conv2d(x.double().unsqueeze(0), w.double(), b.double(), padding=1)[0]
    mag = F.conv2d(x.double().abs().unsqueeze(0), w.double().abs(), b.double().abs(), padding=1)[0]
    err = float((o[:, 1:-1, 1:-1].double() - ref).abs().max())
    print("2-D: max error", err, "bound", 2.0 ** -18 * float(mag.max()))
    assert err < 2.0 ** -18 * float(mag.max())


if __name__ == "__main__":
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "rvc-maker_amd"))
    from rvc_amd import ops as _ops
    _ops._lib.load()
    np.savez(sys.argv[1], **{n: run_case(_ops, n)[0].numpy() for n in CASES})
