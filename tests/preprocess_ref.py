"""Dataset preprocessing (main/inference/preprocess.py:129-185) restated in numpy / scipy: what
``rvc_amd.preprocess`` computes on the device, step for step, for the CPU and GPU tests to compare against.

* ``chain``          -- ``PreProcess.process_audio`` on samples already loaded: lfilter, peak mix, the silence
  slicer, the chunk plan, the f32 slices at ``sr`` and at 16 kHz (``rvc_amd.audio_io.resample``'s polyphase
  filter, as the fixture's generator stubs ``librosa.resample``).
* ``plan_chunks``    -- the ``while 1`` loop of preprocess.py:168-182 as (start, length) pairs.
* ``warmup_rule``    -- the warm-up length the device lfilter derives from ``b, a``.
* ``lfilter_chunked``-- the device lfilter's own arithmetic (chunks rebuilt from a zero state ``warm`` samples
  back, scipy's operation order), vectorised over chunks: what the kernel returns, bit for bit.
* ``resample_plan``  -- scipy's ``resample_poly`` bookkeeping (taps behind their pre-padding, ``n_pre_remove``).
* ``resample_bound`` -- the error bound of an L-term f64 dot product for those taps.
"""
from __future__ import annotations

import numpy as np
from scipy import signal

from rvc_amd import audio_io, edges

OVERLAP, MAX_AMPLITUDE, ALPHA, HIGH_PASS_CUTOFF, SAMPLE_RATE_16K = 0.3, 0.9, 0.75, 48, 16000


def make_slicer(sr):
    return edges.Slicer(sr=sr, threshold=-42, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)


def normalize(audio):
    peak = np.abs(audio).max()
    if peak > 2.5:
        return None
    return (audio / peak * (MAX_AMPLITUDE * ALPHA)) + (1 - ALPHA) * audio


def plan_chunks(seg_len, sr, per):
    """preprocess.py:171-182 for one segment of ``seg_len`` samples -> [(start, length), ...]."""
    out, i = [], 0
    while True:
        start = int(sr * (per - OVERLAP) * i)
        i += 1
        rest = max(seg_len - start, 0)
        if rest > (per + OVERLAP) * sr:
            out.append((start, min(int(per * sr), rest)))
        else:
            out.append((start, rest))
            return out


def segments(slicer, audio):
    """Slicer.slice as (begin, end) sample ranges, and the RMS track it cut by (None for a short input)."""
    n = audio.shape[0]
    if n <= slicer.min_length:
        return [(0, n)], None
    rms = edges.get_rms(audio, slicer.win_size, slicer.hop_size).squeeze(0)
    tags = slicer.silence_tags(rms)
    if not tags:
        return [(0, n)], rms
    h, total = slicer.hop_size, rms.shape[0]
    out = []
    if tags[0][0] > 0:
        out.append((0, min(n, tags[0][0] * h)))
    for a, b in zip(tags[:-1], tags[1:]):
        out.append((a[1] * h, min(n, b[0] * h)))
    if tags[-1][1] < total:
        out.append((tags[-1][1] * h, min(n, total * h)))
    return out, rms


def chain(audio, sr, per, cut_preprocess=True, process_effects=True, filt="lfilter"):
    """-> dict(offsets [n][2] (start, length in the processed audio), rms, gt [f32 slices], k16 [f32 slices])."""
    rms = None
    if process_effects:
        if filt == "lfilter":
            b, a = signal.butter(N=5, Wn=HIGH_PASS_CUTOFF, btype="high", fs=sr)
            audio = signal.lfilter(b, a, audio)
        else:
            sos = signal.butter(N=5, Wn=HIGH_PASS_CUTOFF, btype="high", fs=sr, output="sos")
            audio = signal.sosfilt(sos, np.asarray(audio, np.float64))
        audio = normalize(audio)
    offsets = []
    if cut_preprocess:
        segs, rms = segments(make_slicer(sr), audio)
        for s0, s1 in segs:
            offsets += [(s0 + st, ln) for st, ln in plan_chunks(s1 - s0, sr, per)]
    else:
        offsets.append((0, audio.shape[0]))
    gt = [audio[o: o + n].astype(np.float32) for o, n in offsets]
    k16 = [audio_io.resample(audio[o: o + n], sr, SAMPLE_RATE_16K).astype(np.float32) for o, n in offsets]
    return dict(offsets=np.array(offsets, np.int64).reshape(-1, 2), rms=rms, gt=gt, k16=k16, audio=audio)


def warmup_rule(b, a, tile=32):
    """The first multiple of ``tile`` past the last sample whose |impulse response| is >= 1e-12."""
    x = np.zeros(65536)
    x[0] = 1.0
    h = signal.lfilter(b, a, x)
    last = int(np.flatnonzero(~(np.abs(h) < 1e-12))[-1])
    return ((last + 1) // tile + 1) * tile


def lfilter_chunked(b, a, x, warm, chunk=512):
    """Every chunk of ``chunk`` outputs from a zero state ``warm`` samples before it (zero input before n = 0),
    with scipy's DOUBLE_filt expression; all chunks advance together as numpy vectors."""
    b, a = np.asarray(b, np.float64) / a[0], np.asarray(a, np.float64) / a[0]
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    nch = -(-n // chunk)
    xp = np.concatenate([np.zeros(warm), x, np.zeros(nch * chunk - n)])
    lo = np.arange(nch) * chunk  # window start in xp = lo - warm + warm
    z = np.zeros((5, nch))
    y = np.zeros((nch, chunk))
    for t in range(warm + chunk):
        xn = xp[lo + t]
        yn = z[0] + b[0] * xn
        for i in range(4):
            z[i] = z[i + 1] + xn * b[i + 1] - yn * a[i + 1]
        z[4] = xn * b[5] - yn * a[5]
        if t >= warm:
            y[:, t - warm] = yn
    return y.reshape(-1)[:n]


def resample_plan(up, down):
    """scipy.signal.resample_poly's taps and bookkeeping -> (h behind n_pre_pad zeros, n_pre_remove)."""
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = signal.firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return np.concatenate([np.zeros(n_pre_pad), h]), n_pre_remove


def resample_bound(up, down, xmax):
    """2 L 2^-53 S max|x|: L taps per output phase, S the largest per-phase sum of |h|."""
    h, _ = resample_plan(up, down)
    L = -(-h.size // up)
    hp = np.concatenate([h, np.zeros(L * up - h.size)]).reshape(L, up)
    S = np.abs(hp).sum(axis=0).max()
    return 2 * L * 2.0 ** -53 * S * xmax
