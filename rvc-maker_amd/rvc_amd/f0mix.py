"""hybrid[a+b+...] f0 (``VC.get_f0_hybrid``, main/inference/convert.py:283-302) on the device (csrc/f0mix.hip):
the 0.999 |x| quantile normalisation of the members' input and the resample-and-median mix of their raw tracks.
Which members exist and what each returns is f0.py's (``F0Bank.f0_members``, ``F0Bank.f0_raw``); ``parse_hybrid`` is the
one parser of the method string.
"""
from __future__ import annotations

import ctypes
import re

import torch

from . import _lib, f0, ops

CREPE_MEMBERS = tuple(f0.CREPE_METHODS)
MANGIO_MEMBERS = tuple(f0.MANGIO_METHODS)
# the members that need no model, or one every holder can load (rmvpe.pt, crepe_<capacity>.pth)
MEMBERS = ("rmvpe", f0.RMVPE_LEGACY, "pm", "swipe") + CREPE_MEMBERS + MANGIO_MEMBERS
MAX_TRACKS = 8


def is_hybrid(f0_method: str) -> bool:
    return "hybrid" in f0_method  # the reference's own test (convert.py:306)


def parse_hybrid(f0_method: str, extra=()) -> list[str]:
    """"hybrid[a+b]" -> ["a", "b"] as get_f0_hybrid parses it; a member that is not on the device path raises
    NotImplementedError naming it.  A repeated member stays repeated (the reference computes it again).
    ``extra`` names members the caller accepts beyond MEMBERS (f0.F0Bank.f0_members passes the ones whose model it
    holds: "fcpe", and "fcpe-legacy", whose model it then asks for)."""
    m = re.search(r"hybrid\[(.+)\]", f0_method)
    if not m:
        raise ValueError(f"f0 method {f0_method!r}: expected hybrid[a+b+...]")
    members = [s.strip() for s in m.group(1).split("+")]
    for name in members:
        if name not in MEMBERS and name not in extra:
            f0.refuse("hybrid f0 member", name)
    if len(members) > MAX_TRACKS:
        raise NotImplementedError(f"hybrid f0: {len(members)} members (at most {MAX_TRACKS})")
    return members


def _f32(x):
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 1:
        raise TypeError(f"rvc_amd f0mix: expected a contiguous 1-D CUDA f32 tensor, got {x.dtype} "
                        f"{tuple(x.shape)} on {x.device}")
    return ctypes.c_void_p(x.data_ptr())


QUANTILE_NUMPY, QUANTILE_TORCH = 0, 1  # RVC_QUANTILE_*: whose lerp between the two order statistics


def abs_quantile(x: torch.Tensor, lerp: int = QUANTILE_NUMPY) -> torch.Tensor:
    """np.quantile(np.abs(x), 0.999) of a device f32 signal -> device f32 [1]; QUANTILE_TORCH: torch.quantile's
    value (its lerp is one fused multiply-add; extract.py:166)."""
    lib = _lib.load()
    q = torch.empty(1, dtype=torch.float32, device=x.device)
    need = lib.rvc_abs_quantile_work_bytes()
    work = ops._workspace(x.device, need, "quantile")
    ops.check(lib.rvc_abs_quantile_as(_f32(x), x.numel(), int(lerp), ops._p(work), need, _f32(q), ops._stream()),
              "abs_quantile")
    return q


def normalize(x: torch.Tensor, lerp: int = QUANTILE_NUMPY) -> torch.Tensor:
    """x / np.quantile(np.abs(x), 0.999) in f32 (get_f0_hybrid's and get_f0_mangio_crepe's input normalisation), on
    the device; QUANTILE_TORCH: x / torch.quantile(torch.abs(x), 0.999) (FeatureInput.get_mangio_crepe)."""
    q = abs_quantile(x, lerp)
    out = torch.empty_like(x)
    ops.check(_lib.load().rvc_div_scalar(_f32(x), x.numel(), _f32(q), _f32(out), ops._stream()), "div_scalar")
    return out


def mix(tracks, p_len: int) -> torch.Tensor:
    """Raw member tracks (device f32 or f64, any lengths) -> f64 [p_len]: each resampled as
    np.interp(np.linspace(0, n, p_len), np.arange(n), f0), then np.nanmedian over the members."""
    if not 1 <= len(tracks) <= MAX_TRACKS:
        raise ValueError(f"f0 mix: {len(tracks)} tracks (1..{MAX_TRACKS})")
    arr = (_lib.F0Track * len(tracks))()
    keep = []
    for i, t in enumerate(tracks):
        if not t.is_cuda or t.dtype not in (torch.float32, torch.float64) or t.dim() != 1 or t.numel() == 0:
            raise TypeError(f"rvc_amd f0mix: track {i}: expected a 1-D CUDA f32/f64 tensor, got {t.dtype} "
                            f"{tuple(t.shape)} on {t.device}")
        t = t.contiguous()
        keep.append(t)
        arr[i].f0, arr[i].n, arr[i].is_f64 = t.data_ptr(), t.numel(), int(t.dtype == torch.float64)
    out = torch.empty(p_len, dtype=torch.float64, device=keep[0].device)
    ops.check(_lib.load().rvc_f0_mix(arr, len(tracks), p_len, ctypes.c_void_p(out.data_ptr()), ops._stream()),
              "f0_mix")
    return out
