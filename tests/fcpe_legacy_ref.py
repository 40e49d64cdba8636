"""The Performer (FAVOR+) self-attention and the decode of the fcpe-legacy f0 estimator restated with torch on the
CPU at any dtype: the oracle of the op-level GPU tests (in f64) and, against tests/golden/fcpe_legacy_attn.npz and
fcpe_legacy.npz (the reference's own output), of the CPU test.

Per head, with D = 64 channels, M random features P [M][D], c = D^-0.25 and r = M^-0.5:
queries become q' = r (exp(c q P^T - |c q|^2 / 2 - rowmax(c q P^T)) + 1e-4), keys k' = r exp(c k P^T - |c k|^2 / 2 +
1e-4) (no maximum), and out = q' (k'^T v) / (q' sum_t k' + 1e-8): attention that is linear in the number of frames.
The legacy decode is fcpe's 9-bin local-argmax decoder with no f0 range (fcpe_ref.decode, range open).
"""
import numpy as np
import torch

import fcpe_ref


def features(x, proj, is_query):
    """x [..., T, D], proj [M, D] -> the positive random features [..., T, M]."""
    D, M = x.shape[-1], proj.shape[0]
    c, r = D ** -0.25, M ** -0.5
    dash = (c * x) @ proj.to(x.dtype).T
    diag = (x * x).sum(-1, keepdim=True) / 2.0 * c ** 2
    if is_query:
        return r * (torch.exp(dash - diag - dash.max(dim=-1, keepdim=True).values) + 1e-4)
    return r * torch.exp(dash - diag + 1e-4)


def attention(q, k, v, proj):
    """q, k, v [..., T, D] -> [..., T, D]."""
    qp, kp = features(q, proj, True), features(k, proj, False)
    ctx = kp.transpose(-1, -2) @ v  # [..., M, D]
    den = (qp * kp.sum(dim=-2, keepdim=True)).sum(-1, keepdim=True) + 1e-8
    return (qp @ ctx) / den


def heads(x, H):
    """[..., T, H * D] -> [..., H, T, D]."""
    return x.reshape(*x.shape[:-1], H, x.shape[-1] // H).transpose(-2, -3)


def self_attention(x, w, proj, H=8):
    """SelfAttention on x [T, C] (after the layer's LayerNorm): w maps "to_q.weight", ... , "to_out.bias" to
    tensors (any dtype: cast to x's) -> [T, C]."""
    w = {n: t.to(x.dtype) for n, t in w.items()}
    q, k, v = (heads(x @ w[f"to_{n}.weight"].T + w[f"to_{n}.bias"], H) for n in "qkv")
    o = attention(q, k, v, proj).transpose(-2, -3)
    return o.reshape(x.shape[0], -1) @ w["to_out.weight"].T + w["to_out.bias"]


def decode(latent, cent_table, threshold=0.03):
    """latent f32 [T][C] -> the model's f0 f32 [T]: confidence <= threshold -> 0 and nothing else."""
    return fcpe_ref.decode(latent, cent_table, threshold, 0.0, np.inf)


def f0_f64(latent, cent_table, threshold, p_len, hop_length, sample_rate=16000):
    """The whole tail in f64, as the reference's f64 run computes it from its f64 latent [T][C]: the 9-bin decode
    (the threshold and the cent table are f32 numbers widened), the resize to p_len with unvoiced frames as NaN,
    then compute_f0 / post_process -> (the model's f0 [p_len], the final f0 [p_len])."""
    lat, cent = np.asarray(latent, np.float64), np.asarray(cent_table, np.float64)
    T, C = lat.shape
    am = lat.argmax(axis=1)
    win = np.clip(am[:, None] + np.arange(-4, 5)[None, :], 0, C - 1)
    y = np.take_along_axis(lat, win, axis=1)
    f0 = 10.0 * 2.0 ** ((cent[win] * y).sum(1) / y.sum(1) / 1200.0)
    f0[lat[np.arange(T), am] <= np.float64(np.float32(threshold))] = 0.0
    if p_len != T:
        x = np.where(f0 == 0, np.nan, f0)
        src = np.maximum(T / p_len * (np.arange(p_len) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), T - 1)
        i1 = np.minimum(i0 + 1, T - 1)
        lam = src - i0
        f0 = np.nan_to_num((1.0 - lam) * x[i0] + lam * x[i1], nan=0.0)
    nz = np.flatnonzero(f0)
    if nz.size == 0:
        return f0, np.zeros(p_len)
    if nz.size == 1:
        return f0, np.ones(p_len) * f0[nz[0]]
    return f0, np.interp(np.arange(p_len) * hop_length / sample_rate, hop_length / sample_rate * nz, f0[nz],
                         left=f0[nz[0]], right=f0[nz[-1]])
