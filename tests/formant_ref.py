"""Vectorised f64 NumPy restatement of formant shifting (the phase vocoder at factor 1 that
``load_audio`` runs for ``formant_shifting``), written from the algorithm: every frame at once, the
lifter as two cosine-matrix products, ``cumsum`` for the phase, a strided overlap-add.
``tests/test_formant_cpu.py`` pins it to the reference's own output (``tests/golden/formant.npz``), so
it can serve as the oracle at sizes the fixture does not hold."""
from __future__ import annotations

import numpy as np


def _not_normal(v):
    return ~np.isfinite(v) | (np.abs(v) < np.finfo(np.float64).tiny)


def _envelope(mag, q, n_fft):
    """10 ** (low-quefrency part of log10 |X|): cepstral coefficients 0..q, weights 1, 2..2, 1 on both sides."""
    nb = mag.shape[1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lg = np.log10(mag)
        ang = 2 * np.pi * ((np.arange(nb)[:, None] * np.arange(q + 1)[None, :]) % n_fft) / n_fft
        c = np.cos(ang)  # [bin][coefficient]
        h = np.full(nb, 2.0)
        h[[0, -1]] = 1.0
        w = np.full(q + 1, 2.0)
        w[[0, -1]] = 1.0
        cep = (lg * h) @ c * w
        return 10.0 ** (cep @ c.T / n_fft)


def _resample_rows(env, factor):
    """Each row linearly resampled along the bin axis by ``factor``; bins past the source stay 0."""
    nb = env.shape[1]
    m = int(nb * factor)
    i = np.arange(min(nb, m))
    k = i * (nb / m)
    j = np.trunc(k).astype(int)
    k = k - j
    ok = j < nb - 1
    out = np.zeros_like(env)
    out[:, i[ok]] = k[ok] * env[:, j[ok] + 1] + (1 - k[ok]) * env[:, j[ok]]
    return out


def shiftpitch(x, quefrency=0.0, distortion=1.0, n_fft=1024, hop=32, sr=16000):
    """x [L] (any float dtype) -> the shifted signal in x's dtype."""
    x = np.asarray(x)
    L = x.size
    if L < n_fft:
        raise ValueError("input shorter than one frame")
    M = (L - n_fft) // hop + 1
    nb = n_fft // 2 + 1
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    idx = hop * np.arange(M)[:, None] + np.arange(n_fft)[None, :]
    X = np.fft.rfft(x[idx] * win, axis=-1) / n_fft
    mag, arg = np.abs(X), np.angle(X)

    bins = np.arange(nb)
    freqinc, phaseinc = sr / n_fft, 2 * np.pi * hop / n_fft
    delta = np.diff(arg, axis=0, prepend=np.zeros((1, nb)))
    wrapped = (delta - bins * phaseinc + np.pi) % (2 * np.pi) - np.pi
    freq = (bins + wrapped / phaseinc) * freqinc
    outside = (freq <= 0) | (freq >= sr / 2)

    q = int(quefrency * sr)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if q:
            env = _envelope(mag, q, n_fft)
            mask = _not_normal(env)
            mag = np.where(mask, 0.0, mag / env)
            if distortion != 1:
                env = _resample_rows(np.where(mask, 0.0, env), distortion)
                mask = _not_normal(env)
            mag = np.where(outside, 0.0, mag)
            mag = np.where(mask, 0.0, mag * env)
        else:
            mag = np.where(outside, 0.0, mag)

    phase = np.cumsum((bins + (freq - bins * freqinc) / freqinc) * phaseinc, axis=0)
    Y = mag * np.exp(1j * phase)
    Y[:, [0, -1]] = 0
    frames = np.fft.irfft(Y, n=n_fft, axis=-1) * n_fft * (win * hop / np.sum(win * win))

    y = np.zeros(M * hop + n_fft)
    for r in range(n_fft // hop if n_fft % hop == 0 else 0):  # frames r, r + n_fft / hop, ... do not overlap
        sel = frames[r::n_fft // hop]
        start = r * hop
        y[start:start + sel.size] += sel.reshape(-1)
    if n_fft % hop:
        for m in range(M):
            y[m * hop:m * hop + n_fft] += frames[m]
    y = y[:L] if y.size >= L else np.concatenate([y, np.zeros(L - y.size)])
    return y.astype(x.dtype)


def cases():
    """name -> (f32 input, formant_qfrency, formant_timbre)."""
    from rvc_amd import synthetic
    out = {}
    speech = synthetic.synthetic_audio(1.5, seed=31).astype(np.float32)
    for i, (qf, tb) in enumerate([(0.8, 0.8), (0.8, 1.0), (3.0, 1.4), (16.0, 0.5), (0.05, 0.8)]):
        out[f"speech{i}"] = (speech, qf, tb)
    edge = synthetic.synthetic_audio(0.5, seed=6).astype(np.float32)
    for L in (1024, 1025, 1055, 1056, 2047, 5017):  # M = 1; the M 1 -> 2 boundary; tails the frames do not reach
        out[f"len{L}"] = (edge[:L].copy(), 0.8, 0.8)
    gap = synthetic.synthetic_audio(0.5, seed=5).astype(np.float32)[:6000].copy()
    gap[2000:3600] = 0.0  # digital silence: whole frames of zeros (the NaN-envelope mask)
    for i, (qf, tb) in enumerate([(0.8, 0.8), (0.8, 1.0), (1.0, 1.25)]):
        out[f"gap{i}"] = (gap, qf, tb)
    return out
