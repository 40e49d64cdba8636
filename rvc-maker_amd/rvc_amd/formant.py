"""Formant shifting on the device: drop-in for ``StftPitchShift.shiftpitch`` at ``factors=1``
(``main/library/algorithm/stftpitchshift.py``).

``load_audio`` runs it when ``formant_shifting`` is set (``main/library/utils.py:104-108``:
``StftPitchShift(1024, 32, 16000).shiftpitch(audio, factors=1, quefrency=formant_qfrency * 1e-3,
distortion=formant_timbre)``): a phase vocoder that leaves the pitch where it is and resamples the
cepstral envelope along frequency by ``distortion``.  The whole chain runs in f64 in
``csrc/formant.hip`` like the reference; the host only builds the two windows the reference builds
with NumPy (the periodic Hann and its ``hop / sum(w^2)`` synthesis scaling).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check


def _frame_size(framesize):
    sizes = np.ravel(framesize)
    if int(sizes[0]) != int(sizes[-1]):
        raise NotImplementedError("asymmetric analysis / synthesis windows are not on the load_audio path")
    return int(sizes[0])


def _validate(x, factors, normalization, framesize):
    """The reference's argument checks plus what is out of scope here; no device is touched."""
    n_fft = _frame_size(framesize)
    if np.ravel(np.asarray(factors)).tolist() != [1]:
        raise NotImplementedError("only factors=1 (formant shifting) is on the load_audio path (utils.py:106)")
    if normalization:
        raise NotImplementedError("normalization is not on the load_audio path (utils.py:106)")
    if (x.dim() if torch.is_tensor(x) else np.ndim(x)) != 1:
        raise ValueError("input.ndim != 1")
    if torch.is_tensor(x):
        floating, n = x.is_floating_point(), x.numel()
    else:
        dt = np.asarray(x).dtype
        if np.issubdtype(dt, np.integer):
            raise NotImplementedError("integer PCM input (load_audio passes float samples)")
        floating, n = np.issubdtype(dt, np.floating), np.asarray(x).size
    if not floating:
        raise TypeError("not np.issubdtype(dtype, np.floating)")
    if n < n_fft:  # the reference's sliding_window_view raises the same way
        raise ValueError(f"formant: {n} samples are shorter than one frame of {n_fft}")


class FormantShiftAMD:
    """The shifter's windows on the device, for one (sample rate, frame size, hop) combination."""

    def __init__(self, sample_rate=16000, framesize=1024, hopsize=32, device="cuda"):
        self.sample_rate, self.framesize, self.hopsize = int(sample_rate), _frame_size(framesize), int(hopsize)
        self.device = device
        n = self.framesize
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)  # symmetric_window
        self.win = torch.from_numpy(w).to(device)
        self.synth_win = torch.from_numpy(w * self.hopsize / np.sum(w * w)).to(device)  # istft's W

    def _args(self, quefrency, distortion):
        a = _lib.FormantArgs()
        a.n_fft, a.hop, a.sample_rate = self.framesize, self.hopsize, self.sample_rate
        a.quefrency_samples = int(quefrency * self.sample_rate)  # stftpitchshift.py:211
        a.distortion = float(distortion)
        a.window = ctypes.c_void_p(self.win.data_ptr())
        a.synth_window = ctypes.c_void_p(self.synth_win.data_ptr())
        return a

    def __call__(self, x: torch.Tensor, quefrency: float, distortion: float) -> torch.Tensor:
        """x: device f32 [n] -> shifted f32 [n] (stream-ordered on the current stream); ``quefrency`` in seconds."""
        if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 1:
            raise TypeError("formant: expected a 1-D CUDA float32 tensor")
        x = x.contiguous()
        n = x.numel()
        if n < self.framesize:
            raise ValueError(f"formant: {n} samples are shorter than one frame of {self.framesize}")
        lib = _lib.load()
        a = self._args(quefrency, distortion)
        need = lib.rvc_formant_work_bytes(n, ctypes.byref(a))
        if need < 0:
            raise ValueError(lib.rvc_last_error().decode())
        work = torch.empty((need + 7) // 8, dtype=torch.float64, device=x.device)
        out = torch.empty_like(x)
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        check(lib.rvc_formant_shift(ctypes.c_void_p(x.data_ptr()), n, ctypes.byref(a),
                                    ctypes.c_void_p(work.data_ptr()), work.numel() * 8,
                                    ctypes.c_void_p(out.data_ptr()), stream), "formant_shift")
        return out

    def shiftpitch(self, input, factors=1, quefrency=0, distortion=1, normalization=False):
        """StftPitchShift.shiftpitch (stftpitchshift.py:190).  ``input``: 1-D numpy array or device tensor;
        returns the same kind (numpy in the input's float dtype, like the reference)."""
        _validate(input, factors, normalization, self.framesize)
        if torch.is_tensor(input):
            return self(input.float().to(self.device), quefrency, distortion).to(input.dtype)
        arr = np.asarray(input)
        out = self(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(self.device), quefrency,
                   distortion)
        return out.cpu().numpy().astype(arr.dtype)


def shiftpitch(input, factors=1, quefrency=0, distortion=1, normalization=False, framesize=1024, hopsize=32,
               samplerate=16000, device="cuda"):
    """``StftPitchShift(framesize, hopsize, samplerate).shiftpitch(input, ...)`` on the device.  The arguments
    are checked before anything is placed on the device."""
    _validate(input, factors, normalization, framesize)
    return FormantShiftAMD(samplerate, framesize, hopsize, device).shiftpitch(input, factors, quefrency, distortion,
                                                                              normalization)
