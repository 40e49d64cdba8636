"""An f64 restatement of what rvc_attention_ex computes (include/rvc_amd.h), on the tensors the C ABI takes.

Plain torch on the CPU: no conv, no oracle call, so rk and ev can be any tensors.  tests/test_attention_ref_cpu.py
pins it to oracle.synth._mha (the TextEncoder's rel-pos MHA, synthesizers.py:221-251); the GPU tests compare both
attention kernels with it."""
import torch


def attn_ref64(q, k, v, H, D, scale, rk=None, ev=None, W=0):
    """q, k, v [B][H*D][T]; rk [B][H][2W+1][T] or None; ev [2W+1][D] or None -> (o [B][H*D][T], m [B][H][T],
    l [B][H][T]), all f64.

    S[q][key] = scale * q^T k, + rk[key - q + W][q] where |key - q| <= W; P = softmax over the keys; O = P V,
    + sum_r P[q][q + r - W] * ev[r] over the keys that exist.  m = max_key S and l = sum_key exp(S - m): what the
    kernels leave in ml."""
    B, _, T = q.shape
    qh = q.double().reshape(B, H, D, T).transpose(2, 3)  # [B][H][T][D]
    kh = k.double().reshape(B, H, D, T).transpose(2, 3)
    vh = v.double().reshape(B, H, D, T).transpose(2, 3)
    s = scale * torch.matmul(qh, kh.transpose(2, 3))  # [B][H][query][key]
    idx = torch.arange(T)
    nb = 2 * W + 1
    if rk is not None:
        rk = rk.double().reshape(B, H, nb, T)
        for r in range(nb):
            off = r - W
            lo, hi = max(0, -off), min(T, T - off)
            if hi > lo:
                ii = idx[lo:hi]
                s[:, :, ii, ii + off] += rk[:, :, r, lo:hi]
    m = s.max(-1).values
    e = torch.exp(s - m.unsqueeze(-1))
    l = e.sum(-1)
    p = e / l.unsqueeze(-1)
    o = torch.matmul(p, vh)  # [B][H][T][D]
    if ev is not None:
        band = torch.zeros(B, H, T, nb, dtype=torch.float64)
        for r in range(nb):
            off = r - W
            lo, hi = max(0, -off), min(T, T - off)
            if hi > lo:
                ii = idx[lo:hi]
                band[:, :, ii, r] = p[:, :, ii, ii + off]
        o = o + torch.matmul(band, ev.double().reshape(nb, D))
    return o.transpose(2, 3).reshape(B, H * D, T), m, l
