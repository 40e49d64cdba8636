"""csrc/attention.hip at the edges the other op tests do not reach: sequences shorter than a tile, a fragment or the
band; the relative band across 64-key tile edges, split-KV edges and the sequence end; the band together with split-KV
and with B > 1; ldc != T and separate q / k / v allocations; the (max, sum) the forward and the combine leave in ml.

Every case runs the f32-MFMA kernel (amax_in = None) and the split-fp16 kernel (amax_in = a cell holding max |qkv|
per clip) and compares each with tests/attention_ref.py in f64.  Bounds are the project's own: the f32 kernel within
test_attention_plain's close(rtol=1e-4, atol=1e-5), the fp16 kernel within test_attention_split_f16's
e16 <= 4 e32 + 1e-6 scale; ml's max within 1e-5 max(1, |m|) and its sum within 1e-4 relative.

The harness: q, k and v lie inside device buffers filled with NaN (a guard before and after each tensor, and the pad
columns when ldc > T), so a masked over-read that leaks shows as a NaN; o, ml and a guard around both are pre-filled
with a sentinel, and every word outside o[.., :T] and ml must come back bit-unchanged.  All inside the test's own
allocations.  Each case prints one "attn_edge" line (e32, e16, the fp16 bound, S): profiles/attention_edges.txt."""
import ctypes

import numpy as np
import pytest
import torch

from attention_ref import attn_ref64
from rvc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 128  # floats before and after every tensor (>= 64 + 8: one key tile plus one V octet)
SENTINEL = -12345.671875  # exact in f32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def n_splits(B, H, D, T):
    """The larger of the two kernels' key-split counts, from the workspace query (0 bytes = one split)."""
    a = ops._lib.AttnArgs()
    a.B, a.H, a.D, a.T = B, H, D, T
    need = ops._lib.load().rvc_attention_workspace_bytes(ctypes.byref(a))
    assert need >= 0
    if need == 0:
        return 1
    per = 4 * B * H * T * (D + 2)
    assert need % per == 0
    return need // per


def nan_framed(x, ldc, hs, H, D):
    """x [B][H*D][T] -> a device buffer of NaN holding x as [B][H] heads of D rows with row stride ldc and head stride
    hs (batch stride H * hs), GUARD floats before and after."""
    B, _, T = x.shape
    bs = H * hs
    buf = torch.full((2 * GUARD + B * bs,), float("nan"))
    body = buf[GUARD:GUARD + B * bs].view(B, H, hs)
    body[:, :, :D * ldc].unflatten(2, (D, ldc))[..., :T] = x.reshape(B, H, D, T)
    return buf.to(DEV)


def amax_cell(q, k, v):
    """A |max| cell per clip holding max |q|, |k|, |v| of that clip, as the QKV projection would publish it."""
    B = q.shape[0]
    cell = ops.AmaxSlots(1, DEV, B)
    for b in range(B):
        mx = max(float(t[b].abs().max()) for t in (q, k, v))
        cell.words[b * ops.AMAX_SHARDS] = int(np.float32(mx).view(np.int32))
    return cell


def run_kernel(q, k, v, H, D, scale, f16, rk=None, ev=None, W=0, pad=0, hs_extra=(0, 0, 0), together=True,
               amax_out=False):
    """One rvc_attention_ex call in the NaN / sentinel harness -> (o [B][H*D][T], ml [B][H][2][T], |max| cells or
    None) on the CPU, after the sentinel check.  pad: ldc = T + pad; hs_extra: floats added to q's, k's and v's head
    stride; together: q, k, v in one allocation (else three)."""
    B, E, T = q.shape
    ldc = T + pad
    hs = [D * ldc + e for e in hs_extra]
    if together:
        assert hs_extra == (0, 0, 0)
        parts = [nan_framed(t, ldc, hs[0], H, D) for t in (q, k, v)]
        n = parts[0].numel()
        whole = torch.cat(parts)  # [guard q guard][guard k guard][guard v guard]: one allocation
        bufs = [whole[i * n:(i + 1) * n] for i in range(3)]
    else:
        bufs = [nan_framed(t, ldc, h, H, D) for t, h in zip((q, k, v), hs)]
    dq, dk, dv = (b[GUARD:] for b in bufs)
    n_o, n_ml = B * E * ldc, B * H * 2 * T
    out = torch.full((3 * GUARD + n_o + n_ml,), SENTINEL, device=DEV)
    before = out.view(torch.int32).clone()
    o = out[GUARD:GUARD + n_o]
    ml = out[2 * GUARD + n_o:2 * GUARD + n_o + n_ml]
    cells = ops.AmaxSlots(1, DEV, B) if amax_out else None
    ops.attention(dq, dk, dv, o, B=B, H=H, D=D, T=T, ldc=ldc, q_hs=hs[0], k_hs=hs[1], v_hs=hs[2], o_hs=D * ldc,
                  scale=scale, q_bs=H * hs[0], k_bs=H * hs[1], v_bs=H * hs[2], o_bs=E * ldc,
                  rk=None if rk is None else rk.to(DEV).contiguous(), ev=None if ev is None else ev.to(DEV).contiguous(),
                  ml=ml, W=W, amax_in=amax_cell(q, k, v)[0] if f16 else None, amax_out=None if cells is None else cells[0])
    torch.cuda.synchronize()
    # everything but o[.., :T] and ml is bit-unchanged
    keep = torch.ones(out.numel(), dtype=torch.bool, device=DEV)
    keep[GUARD:GUARD + n_o].view(B, E, ldc)[..., :T] = False
    keep[2 * GUARD + n_o:2 * GUARD + n_o + n_ml] = False
    same = out.view(torch.int32)[keep] == before[keep]
    assert bool(same.all()), f"{int((~same).sum())} words outside o[.., :T] and ml were written"
    oc = o.view(B, E, ldc)[..., :T].cpu()
    mlc = ml.view(B, H, 2, T).cpu()
    assert bool(torch.isfinite(oc).all()), "non-finite output: a masked over-read leaked"
    assert bool(torch.isfinite(mlc).all()), "non-finite (max, sum)"
    return oc, mlc, cells


def check_case(name, q, k, v, H, D, rk=None, ev=None, W=0, split=None, **kw):
    """Both kernels against attn_ref64 within the project's bounds; ml against the reference's (m, l); the form
    (one split / several) through the workspace query.  Returns {kernel: (o, ml)}."""
    B, _, T = q.shape
    scale = D ** -0.5
    S = n_splits(B, H, D, T)
    if split is not None:
        assert (S > 1) == split, f"T = {T} no longer exercises the form the case names (S = {S})"
    ref, m, l = attn_ref64(q, k, v, H, D, scale, rk=rk, ev=ev, W=W)
    mag = ref.abs().max().item()
    res, err = {}, {}
    for kern in ("f32", "f16"):
        o, ml, _ = run_kernel(q, k, v, H, D, scale, kern == "f16", rk=rk, ev=ev, W=W, **kw)
        res[kern] = (o, ml)
        err[kern] = (o.double() - ref).abs().max().item()
    bound16 = 4 * err["f32"] + 1e-6 * mag
    print(f"attn_edge {name} B={B} H={H} D={D} T={T} W={W if rk is not None else '-'} e32={err['f32']:.3e} "
          f"e16={err['f16']:.3e} bound16={bound16:.3e} S={S}")
    assert err["f32"] <= 1e-5 + 1e-4 * mag, (err["f32"], mag)
    assert err["f16"] <= bound16, (err["f16"], err["f32"], mag)
    for kern in ("f32", "f16"):
        ml = res[kern][1].double()
        em = ((ml[:, :, 0] - m).abs() / m.abs().clamp_min(1.0)).max().item()
        el = ((ml[:, :, 1] - l).abs() / l).max().item()
        assert em <= 1e-5, (kern, "max", em)
        assert el <= 1e-4, (kern, "sum", el)
    if T >= 16:  # (below that rounding alone can make the two agree)
        assert not torch.equal(res["f16"][0], res["f32"][0])  # the split-fp16 kernel ran
    return res


def qkv(B, H, D, T, seed):
    g = gen(seed)
    q, k, v = (torch.randn(B, H * D, T, generator=g) for _ in range(3))
    for t in (q, k, v):
        t[:, :, T // 3] *= 4.0  # one loud frame
    return q, k, v


def band(B, H, D, T, W, seed):
    g = gen(seed)
    return torch.randn(B, H, 2 * W + 1, T, generator=g) * 0.5, torch.randn(2 * W + 1, D, generator=g) * 0.5


# ---------------------------------------------------------------- 1. tiny and tile-edge T, no band
TINY_T = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("H,D,T,B", [(H, D, T, 1) for H, D in ((2, 96), (3, 64)) for T in TINY_T]
                         + [(2, 96, 65, 2), (3, 64, 65, 2)])
def test_tiny_and_tile_edge(H, D, T, B):
    q, k, v = qkv(B, H, D, T, 100 + T)
    check_case("tiny", q, k, v, H, D, split=False)


# ---------------------------------------------------------------- 2. band on short sequences and at tile edges
@pytest.mark.parametrize("T,W", [(T, 10) for T in (1, 5, 10, 11, 21, 33, 63, 64, 65, 96, 129)] + [(65, 0), (65, 15)])
def test_band_short_and_tile_edge(T, W):
    H, D = 2, 96
    q, k, v = qkv(1, H, D, T, 200 + T + W)
    rk, ev = band(1, H, D, T, W, 300 + T + W)
    check_case("band", q, k, v, H, D, rk=rk, ev=ev, W=W, split=False)


def test_band_d64():
    """The band at D = 64 (the ABI allows it; the fp16 block then owns 128 queries in two fragments per wave, and the
    band's skip test spans both): T = 193 leaves the last block one query of its second tile."""
    H, D, T, W = 3, 64, 193, 10
    q, k, v = qkv(2, H, D, T, 250)
    rk, ev = band(2, H, D, T, W, 251)
    check_case("band_d64", q, k, v, H, D, rk=rk, ev=ev, W=W, split=False)


# ---------------------------------------------------------------- 3. band, directed
@pytest.mark.parametrize("T", [65, 130, 515])
def test_band_directed_outer_edge(T):
    """rk is +8 on the two outer rows of the band (key = q - W and key = q + W) and 0 elsewhere, so each query's
    softmax rests on those two keys: a band element dropped at a tile, split or sequence boundary is an O(1) error."""
    H, D, W = 2, 96, 10
    g = gen(400 + T)
    q, k, v = (torch.randn(1, H * D, T, generator=g) * 0.5 for _ in range(3))
    rk = torch.zeros(1, H, 2 * W + 1, T)
    rk[:, :, 0] = 8.0
    rk[:, :, 2 * W] = 8.0
    ev = torch.randn(2 * W + 1, D, generator=g) * 0.5
    check_case("directed", q, k, v, H, D, rk=rk, ev=ev, W=W, split=T >= 512)
    # the premise: in the interior the two outer keys hold most of the mass
    _, m, l = attn_ref64(q, k, v, H, D, D ** -0.5, rk=rk, W=W)
    if T > 4 * W:
        assert float(m[:, :, W:T - W].min()) > 4.0


# ---------------------------------------------------------------- 4. band with split-KV
def clips(B, H, D, T, W, seed):
    """q, k, v, rk, ev with each clip its own rk and one clip scaled by 8 (so the clips' |max| cells differ)."""
    q, k, v = qkv(B, H, D, T, seed)
    for t in (q, k, v):
        t[B - 1] *= 8.0
    rk, ev = band(B, H, D, T, W, seed + 1)
    return q, k, v, rk, ev


def check_batch_independent(name, B, H, D, T, W, seed, split):
    q, k, v, rk, ev = clips(B, H, D, T, W, seed)
    res = check_case(name, q, k, v, H, D, rk=rk, ev=ev, W=W, split=split)
    assert (n_splits(1, H, D, T) > 1) == split
    scale = D ** -0.5
    for kern in ("f32", "f16"):
        for b in range(B):
            o1, ml1, _ = run_kernel(q[b:b + 1], k[b:b + 1], v[b:b + 1], H, D, scale, kern == "f16", rk=rk[b:b + 1],
                                    ev=ev, W=W)
            # include/rvc_amd.h: a clip's result does not depend on the other clips of its batch
            assert torch.equal(o1[0], res[kern][0][b]), (kern, b, (o1[0] - res[kern][0][b]).abs().max().item())
            assert torch.equal(ml1[0], res[kern][1][b]), (kern, b)


@pytest.mark.parametrize("T,S", [(515, 2), (1100, 4)])
def test_band_split_kv(T, S):
    """T = 515: kps = 320, the split edge at key 320, the last tile 3 keys.  T = 1100: four splits."""
    H, D, W = 2, 96, 10
    assert n_splits(1, H, D, T) == S
    q, k, v = qkv(1, H, D, T, 500 + T)
    rk, ev = band(1, H, D, T, W, 600 + T)
    check_case("band_split", q, k, v, H, D, rk=rk, ev=ev, W=W, split=True)


@pytest.mark.parametrize("T,B", [(515, 2), (577, 3)])
def test_band_split_kv_batched(T, B):
    check_batch_independent("band_split_batch", B, 2, 96, T, 10, 700 + T, split=True)


# ---------------------------------------------------------------- 5. band with B > 1, single split
def test_band_batched_single_split():
    check_batch_independent("band_batch", 3, 2, 96, 130, 10, 800, split=False)


# ---------------------------------------------------------------- 6. split-KV without band at D = 64
@pytest.mark.parametrize("B", [1, 2])
def test_split_kv_d64(B):
    H, D, T = 12, 64, 515
    assert n_splits(B, H, D, T) == 2
    q, k, v = qkv(B, H, D, T, 900 + B)
    if B > 1:
        for t in (q, k, v):
            t[B - 1] *= 8.0
    check_case("split_d64", q, k, v, H, D, split=True)


# ---------------------------------------------------------------- 7. ldc > T
@pytest.mark.parametrize("H,D,T,W,split", [(2, 96, 65, 10, False), (2, 96, 300, 10, False), (2, 96, 515, 10, True),
                                           (12, 64, 333, None, False)])
def test_ldc_wider_than_T(H, D, T, W, split):
    """ldc = T + 5, head stride D * ldc: the pad columns of q, k, v hold NaN, those of o the sentinel."""
    q, k, v = qkv(1, H, D, T, 1000 + T)
    rk, ev = band(1, H, D, T, W, 1100 + T) if W is not None else (None, None)
    check_case("ldc", q, k, v, H, D, rk=rk, ev=ev, W=W or 0, split=split, pad=5)


@pytest.mark.parametrize("H,D,T,W", [(2, 96, 130, 10), (3, 64, 130, None)])
def test_separate_allocations_unequal_head_strides(H, D, T, W):
    """q, k and v each in an allocation of their own, head strides D * ldc + 0, + 7 and + 16 (NaN between the heads):
    the fp16 kernel's buffer resources span D * ldc from each head's base."""
    q, k, v = qkv(2, H, D, T, 1200 + D)
    rk, ev = band(2, H, D, T, W, 1300 + D) if W is not None else (None, None)
    check_case("separate", q, k, v, H, D, rk=rk, ev=ev, W=W or 0, split=False, pad=5, hs_extra=(0, 7, 16),
               together=False)


# ---------------------------------------------------------------- 8. amax_out
def assert_cell(cell, y, B):
    """cell (B cells) == max |y[b]| for every batch element, exactly (as tests/test_gpu_amax.py)."""
    y = y.reshape(B, -1)
    for b in range(B):
        want = float(y[b].abs().max().item())
        got = ops.amax_value(cell, b)
        assert got == want, (b, got, want)
        assert np.isfinite(got) and got > 0


@pytest.mark.parametrize("name,H,D,T,W,split", [("band", 2, 96, 130, 10, False), ("band_split", 2, 96, 515, 10, True),
                                                ("combine", 12, 64, 515, None, True)])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_amax_out_exact(name, H, D, T, W, split, f16):
    """With ev the band kernel publishes the final values; split without band, the combine does.  B = 2, the second
    clip 8x louder."""
    B = 2
    assert (n_splits(B, H, D, T) > 1) == split
    q, k, v = qkv(B, H, D, T, 1400 + T + H)
    v[1] *= 8.0
    rk, ev = band(B, H, D, T, W, 1500 + T) if W is not None else (None, None)
    o, _, cells = run_kernel(q, k, v, H, D, D ** -0.5, f16, rk=rk, ev=ev, W=W or 0, amax_out=True)
    assert_cell(cells[0], o, B)
