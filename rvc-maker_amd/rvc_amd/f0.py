"""The f0 estimators of the device path, held once for conversion (pipeline.VC) and extraction
(extract.FeatureInputAMD): which methods exist, where their models live, how they are loaded, and what each returns
as a raw track.  Adding an estimator means a name here, a loader and a branch of ``F0Bank.f0_raw`` (plus, for a single
method with a fused post kernel of its own, a branch of ``VC.f0_device``).

The estimator modules are imported inside the loaders: the package imports without a device.
"""
from __future__ import annotations

import os

import torch

PREDICTORS = os.path.join("assets", "models", "predictors")
CREPE_METHODS = {f"crepe-{c}": c for c in ("tiny", "small", "medium", "large", "full")}  # method -> capacity
# mangio-crepe-<capacity>: the same network behind get_f0_mangio_crepe's framing and decode (method -> capacity)
MANGIO_METHODS = {f"mangio-crepe-{c}": c for c in CREPE_METHODS.values()}
RMVPE_LEGACY = "rmvpe-legacy"  # rmvpe with the decoded f0 outside f0_min..f0_max zeroed
METHODS = ("rmvpe", RMVPE_LEGACY, "pm", "swipe", "fcpe", "fcpe-legacy")  # the single methods beside *crepe-*
HYBRID_EXTRA = ("fcpe",)  # hybrid members beyond f0mix.MEMBERS that need a model the holder always has or can load
LEGACY = "fcpe-legacy"  # a method, and a hybrid member, only while its model is at hand (F0Bank._fcpe_legacy)
ON_PATH = ", ".join(m for m in METHODS if m != LEGACY) + \
          f", crepe-*, mangio-crepe-*, {LEGACY} (with its model) and hybrid[...] over them"


def refuse(what, name, why="is not on the device path"):
    """Every refusal of an f0 method or hybrid member, so that the texts cannot drift apart."""
    raise NotImplementedError(f"{what} {name!r} {why}; the path has {ON_PATH}")


class F0Bank:
    """Mixin: the estimators under ``self.rmvpe``, ``self.crepe`` (capacity -> CrepeAMD), ``self.fcpe``,
    ``self.fcpe_legacy``, ``self.pm`` and ``self.swipe``, each the one given to ``_init_f0`` or loaded on first use.
    The holder provides ``self.device``, ``self.f0_min`` and ``self.f0_max``."""

    CREPE_METHODS = CREPE_METHODS
    MANGIO_METHODS = MANGIO_METHODS
    HYBRID_EXTRA = HYBRID_EXTRA
    FCPE_LEGACY_PT = os.path.join(PREDICTORS, "fcpe_legacy.pt")
    MEMBER_ONLY = ()  # methods this holder takes as hybrid members but not alone

    def _init_f0(self, rmvpe=None, crepe=None, fcpe=None, fcpe_legacy=None):
        self.rmvpe = rmvpe
        self.crepe = dict(crepe or {})
        self.fcpe = fcpe
        self.fcpe_legacy = fcpe_legacy
        self.pm = self.swipe = None

    # ------------------------------------------------------------------ loaders
    def _rmvpe(self):
        if self.rmvpe is None:
            from .rmvpe import RMVPEAMD
            self.rmvpe = RMVPEAMD.from_file(os.path.join(PREDICTORS, "rmvpe.pt"), self.device)
        return self.rmvpe

    def _crepe(self, capacity):
        if capacity not in self.crepe:
            from .crepe import CrepeAMD
            self.crepe[capacity] = CrepeAMD.from_file(os.path.join(PREDICTORS, f"crepe_{capacity}.pth"), capacity,
                                                      self.device)
        return self.crepe[capacity]

    def _fcpe(self):
        if self.fcpe is None:
            from .fcpe import FcpeAMD
            self.fcpe = FcpeAMD.from_file(os.path.join(PREDICTORS, "fcpe.pt"), self.device)
        return self.fcpe

    def _fcpe_legacy(self, required=True):
        """The FcpeLegacyAMD held: the one given, or FCPE_LEGACY_PT loaded on first use.  Without either the method
        is off the device path: None, or NotImplementedError when ``required``."""
        if self.fcpe_legacy is None and os.path.exists(self.FCPE_LEGACY_PT):
            from .fcpe_legacy import FcpeLegacyAMD
            self.fcpe_legacy = FcpeLegacyAMD.from_file(self.FCPE_LEGACY_PT, self.device)
        if self.fcpe_legacy is None and required:
            raise NotImplementedError(f"f0 method {LEGACY!r} needs its model: pass fcpe_legacy=FcpeLegacyAMD(...) "
                                      f"or provide {self.FCPE_LEGACY_PT}")
        return self.fcpe_legacy

    def _swipe(self, device=None):
        if self.swipe is None:
            from .swipe import SwipeAMD
            self.swipe = SwipeAMD(device or self.device)
        return self.swipe

    def _pm(self):
        if self.pm is None:
            from .pm import PitchPM
            self.pm = PitchPM(self.device)
        return self.pm

    # ------------------------------------------------------------------ names
    def f0_members(self, f0_method):
        """"hybrid[a+b+...]" -> its members, each one on this holder's path (f0mix.parse_hybrid names the one that is
        not; "fcpe-legacy" without its model raises saying how to supply it)."""
        from . import f0mix
        members = f0mix.parse_hybrid(f0_method, extra=self.HYBRID_EXTRA + (LEGACY,))
        if LEGACY in members:
            self._fcpe_legacy()
        return members

    def check_f0_method(self, f0_method):
        """Raise NotImplementedError, naming it, for a method or hybrid member that is not on the device path; touches
        no device."""
        from . import f0mix
        if f0mix.is_hybrid(f0_method):
            self.f0_members(f0_method)
        elif f0_method == LEGACY:
            self._fcpe_legacy()
        elif f0_method in self.MEMBER_ONLY:
            refuse("f0 method", f0_method, "is taken only as a hybrid member here")
        elif f0_method not in METHODS and f0_method not in CREPE_METHODS and f0_method not in MANGIO_METHODS:
            refuse("f0 method", f0_method)

    # ------------------------------------------------------------------ raw tracks
    def _mangio_scale(self, x32):
        """x / np.quantile(|x|, 0.999) as VC.get_f0_mangio_crepe takes it (NumPy's f32 quantile; rvc_abs_quantile).
        extract.FeatureInputAMD overrides it: get_mangio_crepe divides by torch.quantile."""
        from . import f0mix
        return f0mix.normalize(x32.contiguous())

    def f0_raw(self, x32, member, p_len, hop_length=64, x64=None):
        """One estimator's raw track (before any shift / autotune) on the device f32 signal x32, as the reference's
        members return it: rmvpe f64 [1 + N//160], crepe-* f32 [1 + N//160], pm f64 padded to p_len (Praat reads the
        f64 samples ``x64``, by default x32 promoted), swipe f32 [1 + N//160], fcpe and fcpe-legacy f64 [p_len]
        (the two that read ``hop_length``), rmvpe-legacy as rmvpe, mangio-crepe-* f64 [p_len] (reads ``hop_length``
        too).  ``_mangio_scale`` is the holder's own normalisation of mangio's input."""
        if member == "rmvpe":
            return self._rmvpe().f0_device(x32, 0.03, 0.0, want_f0=True)[2]
        if member == RMVPE_LEGACY:
            # get_f0_rmvpe(legacy=True) (convert.py:248-255): f0[(f0 < f0_min) | (f0 > f0_max)] = 0 in the decode
            return self._rmvpe().f0_device(x32, 0.03, 0.0, want_f0=True, f0_range=(self.f0_min, self.f0_max))[2]
        if member in MANGIO_METHODS:
            # get_f0_mangio_crepe (convert.py:215-228) divides its input by the 0.999 |x| quantile itself: inside a
            # hybrid of the conversion path that is a second division
            return self._crepe(MANGIO_METHODS[member]).f0_mangio(self._mangio_scale(x32), int(hop_length), p_len)
        if member in CREPE_METHODS:
            # shift 2^0 = 1 and no post: pitchf is the raw f0
            return self._crepe(CREPE_METHODS[member]).f0_device(x32, 0.0)[1]
        if member == "pm":
            f0 = self._pm().to_pitch_ac(x32.double() if x64 is None else x64)
            pad = (p_len - f0.numel() + 1) // 2  # get_f0_pm's padding (convert.py:210-212)
            if pad > 0 or p_len - f0.numel() - pad > 0:
                f0 = torch.nn.functional.pad(f0, (pad, p_len - f0.numel() - pad))
            return f0
        if member == "swipe":
            return self._swipe(x32.device).f0(x32)
        if member == "fcpe":
            # get_f0_fcpe (convert.py:239-246): threshold 0.006; the reference truncates f0_min / f0_max and the hop
            return self._fcpe().f0(x32, p_len, int(hop_length), 0.006, int(self.f0_min), int(self.f0_max))
        if member == LEGACY:
            # get_f0_fcpe(legacy=True): threshold 0.03; FCPE_LEGACY never reads f0_min / f0_max
            return self._fcpe_legacy().f0(x32, p_len, int(hop_length), 0.03)
        refuse("hybrid f0 member", member)
