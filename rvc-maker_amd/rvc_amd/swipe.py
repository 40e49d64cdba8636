"""swipe f0 on the device: ``VC.get_f0_swipe`` (main/inference/convert.py:272-276) -- SWIPE' at 16 kHz,
50..1100 Hz, 10 ms frames, strength threshold 0.3 -- followed by get_f0's shift / autotune / f0 file / mel
quantiser (convert.py:308-323) in f32, all in csrc/swipe.hip.

The estimator is f64 on the f32 samples, as the reference computes it.  Its constant tables (pitch candidates,
ERB grid, spline and kernel matrices, pick grids) are built on the host by the library and uploaded once per
``SwipeAMD``.  tests/golden/swipe.npz pins the reference's f0; tests/swipe_ref.py restates the method in numpy.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, ops
from .ops import _p, _pd

NC = 429  # pitch candidates
(T_PC, T_FERBS, T_IDX, T_MU, T_W, T_K, T_WIN, T_TW, T_CMAP, T_CMU, T_PX, T_GRIDX, T_GRIDF0, T_WP, T_KP) = range(15)
_DTYPES = {T_IDX: np.int32, T_CMAP: np.int32, T_GRIDF0: np.float32}


def _p32(t, what="signal"):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1:
        raise TypeError(f"rvc_amd swipe: expected a contiguous 1-D CUDA f32 {what}, got {t.dtype} "
                        f"{tuple(t.shape)} on {t.device}")
    return ctypes.c_void_p(t.data_ptr())


def host_tables():
    """The library's table blob on the host: (uint8 array, lookup(which, window=0) -> array view [rows][cols])."""
    lib = _lib.load()
    blob = np.zeros(lib.rvc_swipe_tables_bytes(), np.uint8)
    ops.check(lib.rvc_swipe_tables(ctypes.c_void_p(blob.ctypes.data), blob.nbytes), "swipe_tables")

    def lookup(which, window=0, padded=False):
        dims = (ctypes.c_int64 * 3)()
        off = lib.rvc_swipe_table_dims(which, window, dims)
        if off < 0:
            raise ValueError(f"swipe table {which} / window {window}")
        rows, cols, ld = dims
        dt = np.dtype(_DTYPES.get(which, np.float64))
        a = blob[off: off + rows * ld * dt.itemsize].view(dt).reshape(rows, ld)
        a = a if padded else a[:, :cols]  # padded: with the columns up to the leading dimension
        return a[0] if rows == 1 else a

    return blob, lookup


class SwipeAMD:
    def __init__(self, device="cuda"):
        blob, _ = host_tables()
        self.tables = torch.from_numpy(blob).to(device)

    def strength(self, x32: torch.Tensor) -> torch.Tensor:
        """x32: device f32 [n] at 16 kHz -> pitch strength S f64 [429][n // 160 + 1]."""
        lib = _lib.load()
        xp = _p32(x32)
        n = x32.numel()
        need = lib.rvc_swipe_work_bytes(n)
        if need < 0:
            raise ValueError(f"swipe: bad signal length {n}")
        work = ops._workspace(x32.device, need, "swipe")
        S = torch.empty(NC, lib.rvc_swipe_frames(n), dtype=torch.float64, device=x32.device)
        ops.check(lib.rvc_swipe_strength(xp, n, _p(self.tables), _p(work), need, _pd(S), ops._stream()),
                  "swipe_strength")
        return S

    def pick(self, S: torch.Tensor) -> torch.Tensor:
        """S: device f64 [429][F] -> f0 f32 [F] (0 = unvoiced)."""
        if not S.is_cuda or S.dtype != torch.float64 or not S.is_contiguous() or S.dim() != 2 or S.shape[0] != NC:
            raise TypeError(f"rvc_amd swipe: expected a contiguous CUDA f64 [429][F] strength, got {S.dtype} "
                            f"{tuple(S.shape)} on {S.device}")
        F = S.shape[1]
        f0 = torch.empty(F, dtype=torch.float32, device=S.device)
        ops.check(_lib.load().rvc_swipe_pick(_pd(S), F, _p(self.tables), _p(f0), ops._stream()), "swipe_pick")
        return f0

    def f0(self, x32: torch.Tensor) -> torch.Tensor:
        """get_f0_swipe: x32 device f32 [n] -> f0 f32 [n // 160 + 1]."""
        return self.pick(self.strength(x32))

    def f0_device(self, x32: torch.Tensor, pitch_shift: float = 0.0, post=None):
        """get_f0(..., "swipe") on the device: (coarse int64 [F], pitchf f32 [F]), F = n // 160 + 1."""
        f0 = self.f0(x32)
        F = f0.numel()
        coarse = torch.empty(F, dtype=torch.int64, device=f0.device)
        pitchf = torch.empty(F, dtype=torch.float32, device=f0.device)
        ops.check(_lib.load().rvc_swipe_post(_p(f0), F, float(2.0 ** (pitch_shift / 12)), ops._post_ref(post, F),
                                             _p(coarse), _p(pitchf), ops._stream()), "swipe_post")
        return coarse, pitchf
