"""Dataset preprocessing on the device: ``main/inference/preprocess.py`` (``PreProcess`` /
``preprocess_training_set``, :129-222), the step that writes the ``sliced_audios`` and ``sliced_audios_16k``
folders ``rvc_amd.extract`` reads.

Per file the reference loads the audio at the training rate, optionally high-passes it (5th-order 48 Hz
Butterworth, ``scipy.signal.lfilter``) and mixes it with its peak-normalised self, optionally denoises it, cuts it
at silences (``Slicer``), cuts every segment into ``per``-second chunks that overlap by 0.3 s, and writes each chunk
as a float32 WAV at the training rate and at 16 kHz.  Here the arithmetic runs in ``csrc/preprocess.hip``:

* ``lfilter``       -- ``rvc_lfilter64``: the filter in f64 over the whole file;
* ``peak_mix``      -- ``rvc_peak_mix64``: max|x| into a device cell and the mix, bit-identical to numpy;
* ``frame_rms``     -- ``rvc_frame_rms64``: the slicer's RMS track (f64 for f32 input too); the track
  is the one read-back the plan needs, and ``edges.Slicer.silence_tags`` turns it into cuts on the host;
* ``resample_poly`` -- ``rvc_resample_poly64``: every chunk of a file to 16 kHz in one launch, each on its own
  samples only (the reference resamples chunk by chunk).  It is ``scipy.signal.resample_poly``, the stand-in for
  ``librosa.resample(res_type="soxr_vhq")`` that ``audio_io.resample`` uses on the host: parity with soxr is
  unpinned, as there.

``load_audio`` and the denoiser are the existing ``audio_io.load_audio`` and ``denoise.reduce_noise``.
"""
from __future__ import annotations

import ctypes
import logging
import math
import os

import numpy as np
import torch
from scipy import signal

from . import _lib, audio_io
from ._lib import check
from .edges import Slicer

log = logging.getLogger(__name__)

OVERLAP, MAX_AMPLITUDE, ALPHA, HIGH_PASS_CUTOFF, SAMPLE_RATE_16K = 0.3, 0.9, 0.75, 48, 16000
AUDIO_EXTENSIONS = ("wav", "mp3", "flac", "ogg", "opus", "m4a", "mp4", "aac", "alac", "wma", "aiff", "webm", "ac3")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _samples(x, what):
    """A 1-D contiguous device tensor of f32 or f64 samples -> (tensor, x_is_f64)."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 1 or x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: expected a 1-D CUDA float32 or float64 tensor")
    return x.contiguous(), int(x.dtype == torch.float64)


def warmup(b, a) -> int:
    """The warm-up length ``rvc_lfilter64`` needs for ``b, a`` (host; raises for a filter past the cap)."""
    b = np.ascontiguousarray(b, np.float64)
    a = np.ascontiguousarray(a, np.float64)
    if b.shape != (6,) or a.shape != (6,):
        raise ValueError("lfilter: order-5 filters only (6 coefficients each)")
    warm = _lib.load().rvc_lfilter64_warmup(ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(a.ctypes.data))
    if warm < 0:
        raise ValueError(f"lfilter: the filter's impulse response does not fall below 1e-12 within "
                         f"{_lib.LFILTER_WARM_CAP} samples")
    return int(warm)


def lfilter(x: torch.Tensor, b, a, warm: int | None = None) -> torch.Tensor:
    """``scipy.signal.lfilter(b, a, x)`` (order 5, zero initial state): device f32 / f64 [n] -> f64 [n]."""
    x, is64 = _samples(x, "lfilter")
    b = np.ascontiguousarray(b, np.float64)
    a = np.ascontiguousarray(a, np.float64)
    if warm is None:
        warm = warmup(b, a)
    n = x.numel()
    lib = _lib.load()
    y = torch.empty(n, dtype=torch.float64, device=x.device)
    need = lib.rvc_lfilter64_work_bytes(n, warm)
    work = torch.empty((need + 7) // 8, dtype=torch.float64, device=x.device) if need > 0 else None
    check(lib.rvc_lfilter64(_ptr(x), is64, n, ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(a.ctypes.data), warm,
                            _ptr(work) if work is not None else None, max(need, 0), _ptr(y), _stream(x)), "lfilter64")
    return y


def frame_rms(x: torch.Tensor, frame_length: int, hop_length: int) -> torch.Tensor:
    """``get_rms(x, frame_length, hop_length)`` (preprocess.py:119-127) -> device f64 [n_frames]."""
    x, is64 = _samples(x, "frame_rms")
    lib = _lib.load()
    n = x.numel()
    frames = lib.rvc_frame_rms64_len(n, frame_length, hop_length)
    if frames < 0:
        raise ValueError(f"frame_rms: n={n} frame_length={frame_length} hop_length={hop_length} must be positive")
    out = torch.empty(frames, dtype=torch.float64, device=x.device)
    check(lib.rvc_frame_rms64(_ptr(x), is64, n, frame_length, hop_length, _ptr(out), _stream(x)), "frame_rms64")
    return out


def peak_mix(x: torch.Tensor, gain: float = MAX_AMPLITUDE * ALPHA, rest: float = 1 - ALPHA):
    """``(x / max|x| * gain) + rest * x`` -> (device f64 [n], device f64 [1] holding max|x|)."""
    x, is64 = _samples(x, "peak_mix")
    if not is64:
        raise TypeError("peak_mix: expected float64 samples (the filter's output)")
    y = torch.empty_like(x)
    peak = torch.empty(1, dtype=torch.float64, device=x.device)
    check(_lib.load().rvc_peak_mix64(_ptr(x), x.numel(), float(gain), float(rest), _ptr(peak), _ptr(y), _stream(x)),
          "peak_mix64")
    return y, peak


def resample_taps(up: int, down: int):
    """scipy.signal.resample_poly's filter and bookkeeping (signaltools.py, ``window=("kaiser", 5.0)``,
    ``padtype="constant"``) -> (taps behind their n_pre_pad zeros, f64; n_pre_remove)."""
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = signal.firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return np.concatenate([np.zeros(n_pre_pad), h]), n_pre_remove


def resample_poly(x: torch.Tensor, up: int, down: int, chunks=None, taps=None):
    """``scipy.signal.resample_poly(x[o: o + n], up, down)`` for every (o, n) of ``chunks`` (default: the whole of
    x) in one launch -> (device f64 [total], device f32 [total], [(out_offset, out_len), ...])."""
    x, is64 = _samples(x, "resample_poly")
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    if chunks is None:
        chunks = [(0, x.numel())]
    h, n_pre_remove = taps if taps is not None else resample_taps(up, down)
    if not torch.is_tensor(h):
        h = torch.from_numpy(np.ascontiguousarray(h, np.float64)).to(x.device)
    seg = np.zeros((len(chunks), 4), np.int64)
    total = 0
    for i, (o, n) in enumerate(chunks):
        m = -(-int(n) * up // down)
        seg[i] = (o, n, total, m)
        total += m
    seg_dev = torch.from_numpy(seg).to(x.device)
    y64 = torch.empty(total, dtype=torch.float64, device=x.device)
    y32 = torch.empty(total, dtype=torch.float32, device=x.device)
    check(_lib.load().rvc_resample_poly64(_ptr(x), is64, x.numel(), _ptr(h), h.numel(), up, down, n_pre_remove,
                                          ctypes.c_void_p(seg.ctypes.data), _ptr(seg_dev), len(chunks), _ptr(y64),
                                          _ptr(y32), total, _stream(x)), "resample_poly64")
    return y64, y32, [(int(s[2]), int(s[3])) for s in seg]


def plan_chunks(seg_len: int, sr: int, per: float):
    """The ``while 1`` loop of preprocess.py:171-182 for one segment -> [(start, length), ...]: chunks of
    ``int(per * sr)`` samples every ``int(sr * (per - OVERLAP) * i)`` while strictly more than
    ``(per + OVERLAP) * sr`` samples remain, then the remainder."""
    out, i = [], 0
    while True:
        start = int(sr * (per - OVERLAP) * i)
        i += 1
        rest = max(seg_len - start, 0)  # len(audio_segment[start:])
        if rest > (per + OVERLAP) * sr:
            out.append((start, min(int(per * sr), rest)))
        else:
            out.append((start, rest))
            return out


def slice_ranges(slicer: Slicer, n: int, tags, total: int):
    """``Slicer.slice``'s chunks (preprocess.py:108-117) as (begin, end) sample ranges of an n-sample signal."""
    if not tags:
        return [(0, n)]
    h = slicer.hop_size
    out = []
    if tags[0][0] > 0:
        out.append((0, min(n, tags[0][0] * h)))
    for a, b in zip(tags[:-1], tags[1:]):
        out.append((a[1] * h, min(n, b[0] * h)))
    if tags[-1][1] < total:
        out.append((tags[-1][1] * h, min(n, total * h)))
    return out


class PreProcessAMD:
    """``PreProcess`` (preprocess.py:129-185) for one training rate and experiment folder."""

    def __init__(self, sr, exp_dir, per, device="cuda"):
        self.slicer = Slicer(sr=sr, threshold=-42, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)
        self.sr = int(sr)
        self.b_high, self.a_high = signal.butter(N=5, Wn=HIGH_PASS_CUTOFF, btype="high", fs=self.sr)
        self.warm = warmup(self.b_high, self.a_high)
        self.per = per
        self.exp_dir = exp_dir
        self.device = device
        g = math.gcd(self.sr, SAMPLE_RATE_16K)
        self.up, self.down = SAMPLE_RATE_16K // g, self.sr // g
        self._taps = None
        self.gt_wavs_dir = os.path.join(exp_dir, "sliced_audios")
        self.wavs16k_dir = os.path.join(exp_dir, "sliced_audios_16k")
        os.makedirs(self.gt_wavs_dir, exist_ok=True)
        os.makedirs(self.wavs16k_dir, exist_ok=True)

    def taps(self):
        if self._taps is None:
            h, n_pre_remove = resample_taps(self.up, self.down)
            self._taps = (torch.from_numpy(h).to(self.device), n_pre_remove)
        return self._taps

    def plan(self, x: torch.Tensor, cut_preprocess: bool):
        """-> ([(offset, length), ...] of the chunks to write, the RMS track read back or None)."""
        n = x.numel()
        if not cut_preprocess:
            return [(0, n)], None
        sl, rms = self.slicer, None
        if n <= sl.min_length:  # Slicer.slice's short-input exit (it compares samples with hops, preprocess.py:65)
            ranges = [(0, n)]
        else:
            rms = frame_rms(x, sl.win_size, sl.hop_size).cpu().numpy()
            ranges = slice_ranges(sl, n, sl.silence_tags(rms), rms.shape[0])
        chunks = []
        for s0, s1 in ranges:
            chunks += [(s0 + start, length) for start, length in plan_chunks(max(s1 - s0, 0), self.sr, self.per)]
        return chunks, rms

    def process_audio(self, path, idx0, sid, cut_preprocess, process_effects, clean_dataset, clean_strength):
        """preprocess.py:155-185.  Returns what it wrote: ``names`` (file names, the same in both folders),
        ``offsets`` int64 [n][2] (start, length of every chunk in the processed audio) and ``rms`` (the slicer's
        track, or None when it was not needed)."""
        try:
            audio = audio_io.load_audio(path, self.sr)
            if audio.size == 0:
                raise ValueError("no samples")
            x = torch.from_numpy(np.ascontiguousarray(audio, np.float32)).to(self.device)
            if process_effects:
                x, peak = peak_mix(lfilter(x, self.b_high, self.a_high, self.warm))
                if float(peak.item()) > 2.5:  # _normalize_audio returns None
                    if clean_dataset or cut_preprocess:
                        raise ValueError("peak above 2.5: the normalised audio is None")
                    log.debug(f"{sid}-{idx0}-0-filtered")
                    return dict(names=[], offsets=np.zeros((0, 2), np.int64), rms=None)
            if clean_dataset:
                from .denoise import reduce_noise
                x = reduce_noise(y=x, sr=self.sr, prop_decrease=clean_strength, device=self.device)
            chunks, rms = self.plan(x, cut_preprocess)
            if any(n <= 0 for _, n in chunks):
                raise ValueError("an empty chunk cannot be resampled")
            host = x.cpu().numpy()
            if self.sr == SAMPLE_RATE_16K:
                y16, spans = host, chunks
            else:
                _, y32, spans = resample_poly(x, self.up, self.down, chunks, self.taps())
                y16 = y32.cpu().numpy()
            names = []
            for idx1, ((o, n), (p, m)) in enumerate(zip(chunks, spans)):
                name = f"{sid}_{idx0}_{idx1}.wav"
                audio_io.write_wav_f32(os.path.join(self.gt_wavs_dir, name), host[o: o + n], self.sr)
                audio_io.write_wav_f32(os.path.join(self.wavs16k_dir, name), y16[p: p + m], SAMPLE_RATE_16K)
                names.append(name)
            return dict(names=names, offsets=np.array(chunks, np.int64).reshape(-1, 2), rms=rms)
        except Exception as e:  # noqa: BLE001 -- preprocess.py:184-185
            raise RuntimeError(f"process_audio failed for {path}: {e}") from e


def list_files(input_root):
    """The walk of preprocess.py:196-208 -> [(path, idx0, sid), ...]: every audio file under ``input_root``
    (sid 0) and its integer-named sub-folders (sid = the name), numbered in walk order.  Folders and files are
    visited in sorted order so that every rank numbers them alike."""
    files, idx = [], 0
    for root, dirs, filenames in os.walk(input_root):
        dirs.sort()
        try:
            sid = 0 if root == input_root else int(os.path.basename(root))
        except ValueError:
            raise ValueError(f"dataset folder names must be integers, got '{os.path.basename(root)}'.") from None
        for f in sorted(filenames):
            if f.lower().endswith(AUDIO_EXTENSIONS):
                files.append((os.path.join(root, f), idx, sid))
                idx += 1
    return files


def preprocess_training_set(input_root, sr, num_processes, exp_dir, per, cut_preprocess, process_effects,
                            clean_dataset, clean_strength, device="cuda", rank=0, world=1):
    """preprocess.py:192-222 for one rank: ``idx0`` numbers all files, the rank takes ``files[rank::world]`` and
    writes its own outputs (as ``rvc_amd.extract`` shards its passes).  ``num_processes`` is the reference's CPU
    pool size; the device does the work here, so it is accepted and ignored.  Returns the names written."""
    pp = PreProcessAMD(sr, exp_dir, per, device)
    files = list_files(input_root)
    names = []
    for path, idx0, sid in files[rank::world]:
        names += pp.process_audio(path, idx0, sid, cut_preprocess, process_effects, clean_dataset,
                                  clean_strength)["names"]
    return names
