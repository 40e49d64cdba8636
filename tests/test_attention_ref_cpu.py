"""tests/attention_ref.py pinned to oracle.synth._mha, which test_oracle.py ties to the reference
(synthesizers.py:221-251).

Both run in f64 here: _mha's own band buffer is a torch.zeros of the default dtype, so the default is f64 while it
runs and every tensor it touches is f64.  The two are then the same sums in a different order; the bound is 1e-12 of
the output scale (f64's 2.2e-16 times reductions over <= 192 channels and <= 130 keys, with room), seven orders below
anything an f32 kernel could hide behind."""
import math

import pytest
import torch

from attention_ref import attn_ref64
from oracle import synth as osy

H, D, W = 2, 96, 10


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 7, 11, 21, 40, 130])
def test_attn_ref64_matches_oracle_mha(T, B):
    C = H * D
    g = torch.Generator().manual_seed(1000 * B + T)
    Wt = {}
    for n in ("q", "k", "v", "o"):
        Wt[f"a.conv_{n}.weight"] = (torch.randn(C, C, 1, generator=g) / math.sqrt(C)).double()
        Wt[f"a.conv_{n}.bias"] = (torch.randn(C, generator=g) * 0.1).double()
    Wt["a.emb_rel_k"] = (torch.randn(1, 2 * W + 1, D, generator=g) * D ** -0.5).double()
    Wt["a.emb_rel_v"] = (torch.randn(1, 2 * W + 1, D, generator=g) * D ** -0.5).double()
    x = torch.randn(B, C, T, generator=g).double()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        want = osy._mha(Wt, "a.", x, torch.ones(1, 1, T, T), H, window=W)
    finally:
        torch.set_default_dtype(old)
    assert want.dtype == torch.float64
    q, k, v = (osy._conv(Wt, f"a.conv_{n}", x) for n in "qkv")
    scale = 1 / math.sqrt(D)
    # rk[b][h][r][t] = scale * sum_d q[b][h][d][t] * Ek[r][d]
    rk = scale * torch.einsum("bhdt,rd->bhrt", q.view(B, H, D, T), Wt["a.emb_rel_k"][0])
    o, m, l = attn_ref64(q, k, v, H, D, scale, rk=rk, ev=Wt["a.emb_rel_v"][0], W=W)
    assert o.dtype == torch.float64 and m.shape == (B, H, T) and l.shape == (B, H, T)
    assert bool((l >= 1).all())  # the largest key contributes exp(0)
    got = osy._conv(Wt, "a.conv_o", o)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(1.0, want.abs().max().item()), err


def test_attn_ref64_plain_is_softmax():
    """Without a band it is softmax(scale q^T k) v, and (m, l) are the softmax's own max and sum."""
    g = torch.Generator().manual_seed(3)
    B, Hh, Dd, T = 2, 3, 64, 19
    q, k, v = (torch.randn(B, Hh * Dd, T, generator=g) for _ in range(3))
    o, m, l = attn_ref64(q, k, v, Hh, Dd, 0.125)
    qh, kh, vh = (t.double().view(B, Hh, Dd, T).transpose(2, 3) for t in (q, k, v))
    s = 0.125 * qh @ kh.transpose(2, 3)
    want = (torch.softmax(s, -1) @ vh).transpose(2, 3).reshape(B, Hh * Dd, T)
    assert (o - want).abs().max().item() <= 1e-14
    assert torch.equal(m, s.max(-1).values)
    assert (l - torch.exp(s - m.unsqueeze(-1)).sum(-1)).abs().max().item() <= 1e-13
