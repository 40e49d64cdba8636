"""The decode and post stages of the fcpe f0 estimator restated in numpy, for the CPU test (against the
reference's own output, tests/golden/fcpe.npz) and as the oracle of the op-level GPU tests.

``decode``: the 9-bin local-argmax decoder, the cents -> Hz map and the confidence / range masks of
main/library/predictors/FCPE.py:451-468, 479-480, 751-756, in f32.  ``post``: the resize to p_len with unvoiced
frames as NaN (:757-759) as torch's CPU kernel evaluates it in f32, then compute_f0 / post_process (:975-1000)
in f64.
"""
import numpy as np

f32 = np.float32


def _fma32(a, b, c):
    """A fused multiply-add of f32 operands: the product is exact in f64 and the sum rounds to f32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def decode(latent, cent_table, threshold=0.006, f0_min=50, f0_max=1100):
    """latent f32 [T][C] (after the sigmoid), cent_table f32 [C] -> f0 f32 [T], 0 = unvoiced."""
    latent, cent_table = np.asarray(latent, f32), np.asarray(cent_table, f32)
    T, C = latent.shape
    am = latent.argmax(axis=1)  # the first index of the largest value, as torch.max
    conf = latent[np.arange(T), am]
    win = np.clip(am[:, None] + np.arange(-4, 5)[None, :], 0, C - 1)  # a clamped bin counts again
    y = np.take_along_axis(latent, win, axis=1)
    num, den = np.zeros(T, f32), np.zeros(T, f32)
    for k in range(9):  # a sequential f32 sum
        num = (num + (cent_table[win[:, k]] * y[:, k]).astype(f32)).astype(f32)
        den = (den + y[:, k]).astype(f32)
    cents = (num / den).astype(f32)
    f0 = (f32(10) * np.exp2((cents / f32(1200)).astype(f32)).astype(f32)).astype(f32)
    f0[conf <= f32(threshold)] = 0  # cents * -inf -> 10 * 2^-inf
    f0[f0 < f32(f0_min)] = 0
    f0[f0 > f32(f0_max)] = f32(f0_max)
    return f0


def resize(f0, p_len):
    """F.interpolate(where(f0 == 0, nan, f0), size=p_len, mode="linear") then nan -> 0, f32: torch copies when the
    sizes agree; otherwise its CPU kernel takes the source index fma(T / p_len, i + 0.5, -0.5) clamped at 0 and
    fma(w0, x0, w1 * x1), so a NaN neighbour makes the frame NaN even under a zero weight."""
    f0 = np.asarray(f0, f32)
    T = f0.size
    if p_len == T:
        return f0.copy()
    x = np.where(f0 == 0, f32(np.nan), f0).astype(f32)
    i = np.arange(p_len).astype(f32)
    src = _fma32(np.full(p_len, f32(T) / f32(p_len), f32), i + f32(0.5), np.full(p_len, f32(-0.5)))
    src = np.where(src < 0, f32(0), src).astype(f32)
    i0 = np.minimum(src.astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    lam = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    with np.errstate(invalid="ignore"):
        r = _fma32(f32(1) - lam, x[i0], (lam * x[i1]).astype(f32))
    return np.where(np.isnan(r), f32(0), r).astype(f32)


def post(f0, p_len, hop_length=160, sample_rate=16000):
    """The model's f0 f32 [T] -> FCPE.compute_f0's return, f64 [p_len]."""
    g = resize(f0, p_len)
    nz = np.flatnonzero(g)
    if nz.size == 0:
        return np.zeros(p_len)
    if nz.size == 1:
        return np.ones(p_len) * g[nz[0]]
    return np.interp(np.arange(p_len) * hop_length / sample_rate, hop_length / sample_rate * nz, g[nz],
                     left=g[nz[0]], right=g[nz[-1]])
