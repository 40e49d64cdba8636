"""Mel filterbank for RMVPE's MelSpectrogram (``RMVPE.py:151``).

The reference calls ``librosa.filters.mel(sr=16000, n_fft=1024, n_mels=128,
fmin=30, fmax=8000, htk=True)`` (Slaney area normalisation, float32 output).
librosa is not installed in this image, so this is a restatement of its
published algorithm (librosa 0.10 ``filters.mel`` / ``mel_frequencies`` /
``hz_to_mel(htk=True)``): triangular filters between consecutive mel points,
f64 arithmetic, cast to float32 on store.  Parity vs librosa itself is
UNPINNED (no librosa output exists in the reference tree); everything
downstream of the basis is pinned by the golden vectors, which were generated
with this same basis standing in for librosa.
"""
from __future__ import annotations

import numpy as np


def hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


# Slaney's auditory-toolbox scale (librosa's default, htk=False): linear below 1 kHz at 200/3 Hz per mel,
# logarithmic above with 27 steps per factor 6.4
_F_SP = 200.0 / 3
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel_slaney(f):
    f = np.atleast_1d(np.asarray(f, dtype=np.float64))
    mels = f / _F_SP
    log_t = f >= _MIN_LOG_HZ
    mels[log_t] = _MIN_LOG_MEL + np.log(f[log_t] / _MIN_LOG_HZ) / _LOGSTEP
    return mels


def mel_to_hz_slaney(m):
    m = np.atleast_1d(np.asarray(m, dtype=np.float64))
    freqs = _F_SP * m
    log_t = m >= _MIN_LOG_MEL
    freqs[log_t] = _MIN_LOG_HZ * np.exp(_LOGSTEP * (m[log_t] - _MIN_LOG_MEL))
    return freqs


def mel_filterbank(sr=16000, n_fft=1024, n_mels=128, fmin=30.0, fmax=8000.0, htk=True) -> np.ndarray:
    """``htk=True``: the HTK scale RMVPE asks for; ``htk=False``: the Slaney scale of librosa's defaults, which
    FCPE's ``MelModule`` takes (FCPE.py:833).  Both with Slaney's area normalisation, as librosa's default norm."""
    n_bins = 1 + n_fft // 2
    weights = np.zeros((n_mels, n_bins), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    if htk:
        mel_f = mel_to_hz_htk(np.linspace(hz_to_mel_htk(fmin), hz_to_mel_htk(fmax), n_mels + 2))
    else:
        mel_f = mel_to_hz_slaney(np.linspace(hz_to_mel_slaney(fmin)[0], hz_to_mel_slaney(fmax)[0], n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights
