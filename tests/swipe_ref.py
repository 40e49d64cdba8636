"""SWIPE' f0 in matrix form, f64 numpy + scipy: the restatement the swipe tests compare the device against.

For the only settings the conversion path uses (16 kHz, 50..1100 Hz, 10 ms frames, threshold 0.3) the method
is, per window size ws in (2048, 1024, 512, 256, 128) with hop ws/2:

    A = |rfft(frames * hann)| / sum(hann)         frames of the signal padded by ws/2 zeros in front, ws behind
    L = sqrt(max(0, W @ A)),  L /= ||L||_2        W = the not-a-knot cubic spline onto the ERB grid, a matrix
    S_ws = K @ L                                  K = prime-harmonic cosine kernels of the served candidates

then S = sum_ws mu_ws * interp_time(S_ws), and a per-frame pick (argmax, threshold, parabola, 1/768-octave
grid).  tests/golden/swipe.npz pins ``f0`` to the reference implementation frame for frame
(test_swipe_cpu.py); the device is then compared against ``strength`` / ``pick`` here.
"""
import functools

import numpy as np
from scipy import interpolate

FS = 16000
NC, NE = 429, 328
WS = (2048, 1024, 512, 256, 128)
THR = 0.3


def _harmonics(n):
    """The harmonic numbers a kernel uses besides 1: the primes <= n, and n itself when it is the square of a
    prime (the reference's sieve stops striking multiples at num < sqrt(n), so p * p == n survives)."""
    out = [v for v in range(2, n + 1) if all(v % p for p in range(2, int(v ** 0.5) + 1))]
    r = int(round(n ** 0.5))
    if n >= 4 and r * r == n and r in out:
        out.append(n)
    return out


def _kernel(ferbs, pc):
    q = ferbs / pc
    k = np.zeros(len(ferbs))
    for h in [1] + _harmonics(int(np.fix(ferbs[-1] / pc - 0.75))):
        a = np.abs(q - h)
        peak = a < 0.25
        k[peak] = np.cos(2 * np.pi * q[peak])
        side = (0.25 < a) & (a < 0.75)
        k[side] = k[side] + np.cos(2 * np.pi * q[side]) / 2
    k *= np.sqrt(1 / ferbs)
    return k / np.linalg.norm(k[k > 0])


@functools.lru_cache(maxsize=1)
def tables():
    """pc [429], ferbs [328], and per window size: idx (served candidates), mu, W [328][ws/2+1], K [nc][328]."""
    log2pc = np.arange(np.log2(50.0) * 96, np.log2(1100.0) * 96)
    log2pc *= 1 / 96
    pc = 2 ** log2pc
    d = 1 + log2pc - np.log2(8 * FS / WS[0])
    erb = lambda hz: 21.4 * np.log10(1 + hz / 229)  # noqa: E731
    ferbs = (10 ** (np.arange(erb(pc[0] / 4), erb(FS / 2), 0.1) / 21.4) - 1) * 229
    assert len(pc) == NC and len(ferbs) == NE
    per = []
    for i, ws in enumerate(WS):
        rel = d - (i + 1)
        if i == len(WS) - 1:
            idx = np.where(rel > -1)[0]
            taper = rel[idx] < 0
        elif i == 0:
            idx = np.where(rel < 1)[0]
            taper = rel[idx] > 0
        else:
            idx = np.where(np.abs(rel) < 1)[0]
            taper = np.ones(len(idx), bool)
        mu = np.ones(len(idx))
        mu[taper] = 1 - np.abs(d[idx[taper]] - i - 1)
        f = np.arange(ws // 2 + 1) * (FS / ws)
        W = interpolate.interp1d(f, np.eye(len(f)), kind="cubic", axis=0)(ferbs)
        K = np.stack([_kernel(ferbs, pc[c]) for c in idx])
        per.append(dict(ws=ws, idx=idx, mu=mu, W=W, K=K))
    return pc, ferbs, per


def n_frames(n):
    return n // 160 + 1


def strength(x32):
    """x32: f32 [n] -> S f64 [429][n // 160 + 1]."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    n = len(x)
    pc, _, per = tables()
    t = np.arange(n_frames(n)) * 0.01
    S = np.zeros((NC, len(t)))
    for tab in per:
        ws = tab["ws"]
        hop = ws // 2
        nfr = n // hop + 2
        xp = np.concatenate([np.zeros(hop), x, np.zeros(ws)])
        frames = np.lib.stride_tricks.sliding_window_view(xp, ws)[::hop][:nfr]
        win = np.hanning(ws + 2)[1:-1]
        A = np.abs(np.fft.rfft(frames * win, axis=1) / win.sum()).T            # [bin][frame]
        L = np.sqrt(np.maximum(0, tab["W"] @ A))
        den = np.sqrt(np.sum(L * L, axis=0))
        L = L / np.where(den == 0, 2.220446049250313e-16, den)
        Si = tab["K"] @ L                                                      # [cand][frame]
        ti = np.arange(nfr) * hop / FS
        Si = interpolate.interp1d(ti, Si)(t)
        S[tab["idx"]] = S[tab["idx"]] + tab["mu"][:, None] * Si
    return S


def pick(S):
    """S f64 [429][F] -> f0 f32 [F]."""
    pc = tables()[0]
    out = np.zeros(S.shape[1])
    for k in range(S.shape[1]):
        i = int(np.argmax(S[:, k]))
        if S[i, k] < THR:
            continue
        if i == 0 or i == NC - 1:
            out[k] = pc[0]
            continue
        tc = 1 / pc[i - 1:i + 2]
        c = np.polyfit((tc / tc[1] - 1) * 2 * np.pi, S[i - 1:i + 2, k], 2)
        lo = np.log2(pc[i - 1])
        grid = 2 ** np.arange(lo, np.log2(pc[i + 1]) + 1 / 12 / 64, 1 / 12 / 64)
        val = np.polyval(c, ((1 / grid) / tc[1] - 1) * 2 * np.pi)
        out[k] = 2 ** (lo + np.argmax(val) / 12 / 64)
    return out.astype(np.float32)


def f0(x32):
    return pick(strength(x32))


def get_f0_post_f32(f0_raw, pitch=0.0, autotune_strength=None, rep=None, rep_off=0):
    """get_f0's steps after the estimator on an f32 f0 (autotune, shift, f0 file, mel quantiser) as NumPy 2
    evaluates them for an f32 array -> (coarse int64, pitchf f32)."""
    notes = [49.00, 51.91, 55.00, 58.27, 61.74, 65.41, 69.30, 73.42, 77.78, 82.41, 87.31, 92.50, 98.00, 103.83,
             110.00, 116.54, 123.47, 130.81, 138.59, 146.83, 155.56, 164.81, 174.61, 185.00, 196.00, 207.65, 220.00,
             233.08, 246.94, 261.63, 277.18, 293.66, 311.13, 329.63, 349.23, 369.99, 392.00, 415.30, 440.00, 466.16,
             493.88, 523.25, 554.37, 587.33, 622.25, 659.25, 698.46, 739.99, 783.99, 830.61, 880.00, 932.33, 987.77,
             1046.50]
    f = np.array(f0_raw, np.float32)
    if autotune_strength is not None:
        tuned = np.zeros_like(f)
        for i, v in enumerate(f):
            near = min(notes, key=lambda nt: abs(nt - v))
            tuned[i] = v + (near - v) * autotune_strength
        f = tuned
    f *= pow(2, pitch / 12)
    if rep is not None:
        seg = f[rep_off:rep_off + len(rep)]
        f[rep_off:rep_off + len(rep)] = rep[:seg.shape[0]]
    mel_min, mel_max = 1127 * np.log(1 + 50 / 700), 1127 * np.log(1 + 1100 / 700)
    mel = 1127 * np.log(1 + f / 700)
    mel[mel > 0] = (mel[mel > 0] - mel_min) * 254 / (mel_max - mel_min) + 1
    mel[mel <= 1] = 1
    mel[mel > 255] = 255
    return np.rint(mel).astype(np.int64), f.copy()
