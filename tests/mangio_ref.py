"""mangio-crepe-<capacity> f0 (``VC.get_f0_mangio_crepe``, convert.py:215-228; ``FeatureInput.get_mangio_crepe``,
extract.py:162-171) restated on numpy, from the network's output on.  Test infrastructure only.

The network and the framing are ``oracle.crepe``'s (imported, not restated again).  What differs from crepe-<capacity>:

* ``segments``      ``predict(batch_size = 2 * hop_length)`` postprocesses per batch, so the Viterbi restarts at every
                    batch boundary: offsets ``range(0, T, 2 * hop_length) + [T]``
* ``postprocess``   per segment: fmin / fmax mask, softmax, Viterbi, bins -> Hz with the dither drawn in frame order;
                    no periodicity, no mean / median, no gate.  bins -> Hz comes in two forms (``bins_to_hz``): torch
                    itself per batch, host-dependent in each batch's tail frames, and ``pow2_vector`` throughout
* ``resample``      ``source[source < 0.001] = nan`` and ``np.nan_to_num(np.interp(...))`` onto p_len frames
* ``scale_convert`` the conversion path's ``np.quantile(np.abs(x), 0.999)`` (NumPy 2 on an f32 array: rank, gamma and
                    lerp in f32) and ``scale_extract``, the extraction path's ``torch.quantile(torch.abs(x), 0.999)``
                    (ATen's CPU kernel: the same rank and order statistics, each lerp branch one fused multiply-add).
                    The two differ in the last bit of about one vector in a hundred.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import crepe as ocr
from oracle import pipeline as opl

F0_MIN, F0_MAX = 50, 1100


def variants() -> dict:
    """make_golden_f0_paths.VARIANTS: name -> (pitch, autotune, strength, f0 file), the three get_f0 variants the
    goldens record."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "make_golden_f0_paths", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                             "make_golden_f0_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VARIANTS


def segments(T: int, hop_length: int) -> list[int]:
    return list(range(0, T, 2 * hop_length)) + [T]


def viterbi_bins(probs: np.ndarray, offsets) -> np.ndarray:
    """probs f32 [T][360] (sigmoid outputs, unmasked) -> Viterbi bins int64 [T], each segment decoded alone."""
    p = torch.from_numpy(np.ascontiguousarray(probs.T))[None].clone()  # [1][360][T]
    p[:, :ocr.frequency_to_bins(torch.tensor(F0_MIN))] = -float("inf")
    p[:, ocr.frequency_to_bins(torch.tensor(F0_MAX), torch.ceil):] = -float("inf")
    tr = ocr._transition()
    out = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        sm = torch.softmax(p[:, :, a:b], dim=1)[0].numpy()
        out.append(ocr.viterbi_librosa(sm, tr).astype(np.int64))
    return np.concatenate(out)


def _fma(x, y, z):
    """fl32(x y + z), element-wise and exact: the product of two f32 is exact in f64; where the f64 sum falls exactly
    midway between two f32 values, its own rounding error (TwoSum) breaks the tie."""
    p, z = x.astype(np.float64) * y.astype(np.float64), z.astype(np.float64)
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(r64 < s, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    o64 = other.astype(np.float64)
    swap = (err != 0) & (r64 != s) & (np.abs(r64 - s) == np.abs(o64 - s)) & ((o64 > s) == (err > 0))
    return np.where(swap, other, r)


def pow2_vector(y: np.ndarray) -> np.ndarray:
    """2 ** y in f32 as the VECTOR path of torch's CPU pow evaluates it on x86 hosts with fused multiply-add (its
    1-ulp vector math routine), restated in NumPy so that the value depends on neither the host nor the tensor's length.
    torch sends only whole vector blocks of a tensor through that routine; the remaining tail of each call goes through
    the C library's powf, which differs from it in the last bit of about 2 % of values."""
    f = np.float32
    y = np.asarray(y, f)
    k = lambda v: np.full_like(y, v)  # noqa: E731
    lx, ly = k(0.69314718246459960938), k(-1.904654323148236017e-09)
    dx = lx * y
    dy = _fma(ly, y, _fma(lx, y, -dx))
    q = np.rint((dx + dy) * f(1.442695040888963407359924681001892137426645954152985934135449406931))

    def add2(ax, ay, b):
        rx = ax + b
        v = rx - ax
        return rx, ((ax - (rx - v)) + (b - v)) + ay

    sx, sy = add2(dx, dy, q * f(-0.693145751953125))
    sx, sy = add2(sx, sy, q * f(-1.428606765330187045e-06))
    nx = sx + sy
    sx, sy = nx, sx - nx + sy
    u = k(0.00136324646882712841033936)
    for c in (0.00836596917361021041870117, 0.0416710823774337768554688, 0.166665524244308471679688,
              0.499999850988388061523438):
        u = _fma(u, sx, k(c))
    qx = sx * sx
    qy = _fma(sx + sx, sy, _fma(sx, sx, -qx))
    mx = qx * u
    my = _fma(qy, u, _fma(qx, u, -mx))
    tx = sx + mx
    ty = sx - tx + mx + sy + my
    ox = f(1) + tx
    oy = f(1) - ox + tx + ty
    return np.ldexp(ox + oy, q.astype(np.int32)).astype(f)


def bins_to_hz(bins: np.ndarray, dither: np.ndarray, offsets=None, vector=False) -> np.ndarray:
    """CREPE.py:117-119, f32: 10 * 2 ** ((20 bins + 1997.379 + dither) / 1200).

    ``vector`` False: torch itself, one call per batch [offsets[i], offsets[i + 1]) as ``predict`` makes them -- the
    reference as it runs on this host, the scalar tail of every batch included.  ``vector`` True: every frame through
    ``pow2_vector`` -- what the device computes (rvc_crepe_decode_as, RVC_CREPE_HZ_TORCH), whatever the host and the
    batch lengths.  The two differ only on a batch's tail frames, and there only where the two powers of two do."""
    dither = np.asarray(dither, np.float64)[: len(bins)]
    if vector:
        cents = (20 * bins).astype(np.float32) + np.float32(1997.3794084376191)
        return np.float32(10) * pow2_vector((cents + dither.astype(np.float32)) / np.float32(1200))
    out = []
    offsets = [0, len(bins)] if offsets is None else offsets
    for a, b in zip(offsets[:-1], offsets[1:]):
        cents = ocr.CENTS_PER_BIN * torch.from_numpy(bins[a:b]) + 1997.3794084376191
        out.append((10 * 2 ** ((cents + cents.new_tensor(dither[a:b])) / 1200)).numpy())
    return np.concatenate(out)


def postprocess(probs: np.ndarray, hop_length: int, dither: np.ndarray, vector=False):
    """-> (bins int64 [T], source f32 [T]) of predict(batch_size = 2 * hop_length); ``vector`` as in bins_to_hz."""
    seg = segments(probs.shape[0], hop_length)
    bins = viterbi_bins(probs, seg)
    return bins, bins_to_hz(bins, dither, seg, vector).astype(np.float32)


def resample(source: np.ndarray, p_len: int) -> np.ndarray:
    """convert.py:226-228 on an f32 source [T] -> f64 [p_len]."""
    source = np.array(source, dtype=np.float32)
    source[source < 0.001] = np.nan
    return np.nan_to_num(np.interp(np.arange(0, len(source) * p_len, len(source)) / p_len,
                                   np.arange(0, len(source)), source))


def f0(probs: np.ndarray, hop_length: int, dither: np.ndarray, p_len: int, vector=False) -> np.ndarray:
    """get_f0_mangio_crepe's return from the network's output on; ``vector`` as in bins_to_hz."""
    return resample(postprocess(probs, hop_length, dither, vector)[1], p_len)


def get_f0(track: np.ndarray, pitch, autotune_strength=None, inp_f0=None, x_pad=0):
    """VC.get_f0's tail on the f64 track (convert.py:308-323) -> (coarse int32, pitchf f64)."""
    return opl.coarse_f0(np.array(track, dtype=np.float64), pitch, opl.Consts(40000, x_pad=x_pad), autotune_strength,
                         inp_f0)


def _order_stats(x: np.ndarray):
    """The two order statistics of |x| around rank 0.999 (n - 1) and the weight between them, all in f32."""
    a = np.sort(np.abs(np.asarray(x, np.float32)))
    n = a.size
    virt = np.float32(n - 1) * np.float32(0.999)
    lo = np.floor(virt)
    k0 = int(lo)
    return a[k0], a[min(k0 + 1, n - 1)], np.float32(virt - lo)


def scale_convert(x: np.ndarray) -> np.float32:
    """np.quantile(np.abs(x), 0.999) of f32 x: NumPy's _lerp, every step rounded to f32."""
    a, b, g = _order_stats(x)
    d = np.float32(b - a)
    if g >= np.float32(0.5):
        return np.float32(b - np.float32(d * np.float32(np.float32(1) - g)))
    return np.float32(a + np.float32(d * g))


def _fma32(x, y, z) -> np.float32:
    """fl32(x y + z) for f32 operands: the product is exact in f64; the f64 sum's rounding error (TwoSum) breaks the
    tie when that sum falls exactly midway between two f32 values."""
    p, z = np.float64(x) * np.float64(y), np.float64(z)
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    r = np.float32(s)
    if err != 0 and np.float64(r) != s:
        other = np.nextafter(r, np.float32(np.inf) if np.float64(r) < s else np.float32(-np.inf))
        if abs(np.float64(r) - s) == abs(np.float64(other) - s) and (np.float64(other) > s) == (err > 0):
            r = other
    return r


def scale_extract(x: np.ndarray) -> np.float32:
    """torch.quantile(torch.abs(x), 0.999) of f32 x on the CPU: lerp = fma(w, b - a, a) for w < 0.5, else
    fma(w - 1, b - a, b)."""
    a, b, g = _order_stats(x)
    d = np.float32(b - a)
    if g < np.float32(0.5):
        return _fma32(g, d, a)
    return _fma32(np.float32(g - np.float32(1)), d, b)
