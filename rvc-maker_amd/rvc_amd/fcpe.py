"""fcpe f0 on the device: ``VC.get_f0_fcpe`` (main/inference/convert.py:239-246) -- the conv-only
``CFNaiveMelPE`` of main/library/predictors/FCPE.py at 16 kHz, threshold 0.006, 50..1100 Hz -- followed by
get_f0's shift / autotune / f0 file / mel quantiser (convert.py:308-323, ``rvc_pm_post``).

The mel front end, GroupNorm, the Conformer block's GLU / depthwise conv / SiLU, the local-argmax decoder and
the post-processing are csrc/fcpe.hip; the dense convs run on the conv engine in f32-accurate arithmetic (the
6-pass split-bf16 form: f0 is a per-frame argmax and threshold decision) and the LayerNorms are
``rvc_layernorm_cf``.  Nothing on the f0 path synchronises with the host.  tests/golden/fcpe.npz pins the
reference's output on synthetic weights; tests/fcpe_ref.py restates the decode and post stages in numpy.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, melbasis, ops
from .ops import ACT_SIGMOID, Conv

GLU_TILE = 256  # RVC_GLU_DW_TILE
PRECISION = "fp32x6"
MEL_GEOMETRY = {"num_mels": 128, "n_fft": 1024, "win_size": 1024, "hop_size": 160, "fmin": 0, "fmax": 8000}
MEL_DEFAULTS = dict(MEL_GEOMETRY, sr=16000)  # spawn_wav2mel's defaults for absent fields (FCPE.py:153)


def _pv(t):
    return ctypes.c_void_p(t.data_ptr())


def _check_config(cfg):
    mel, model = cfg.get("mel") or {}, cfg.get("model") or {}
    if not model.get("conv_only"):
        raise NotImplementedError("fcpe: conv_only=False (the attention model: the reference cannot construct it "
                                  "either, FCPE.py:492)")
    if str(mel.get("type")).lower() == "stft":
        raise NotImplementedError("fcpe: mel.type == 'stft' is not on the MI355X path")
    got = {k: (MEL_DEFAULTS[k] if mel.get(k) is None else mel[k]) for k in MEL_DEFAULTS}
    if got["sr"] != 16000:
        raise NotImplementedError(f"fcpe: mel.sr = {got['sr']} (16000 is on the MI355X path)")
    for k, v in MEL_GEOMETRY.items():
        if got[k] != v:
            raise NotImplementedError(f"fcpe: mel.{k} = {got[k]} (the kernels take "
                                      "128 / 1024 / 1024 / 160 / 0 / 8000)")
    if model.get("out_dims", 360) != 360:
        raise NotImplementedError(f"fcpe: model.out_dims = {model.get('out_dims')}")
    return model


class FcpeAMD:
    def __init__(self, ckpt: dict, device="cuda"):
        model = _check_config(ckpt["config_dict"])
        sd = {k: v.float() for k, v in ckpt["model"].items()}
        self.device = device
        self.C, self.n_layers = int(model["hidden_dims"]), int(model["n_layers"])
        C = self.C
        if sd["input_stack.0.weight"].shape != (C, 128, 3) or C % 4 or C > 2048:
            raise ValueError(f"fcpe: hidden_dims {C} does not match the checkpoint")

        def dev(name):
            return sd[name].contiguous().to(device)

        self.basis = torch.from_numpy(melbasis.mel_filterbank(16000, 1024, 128, 0, 8000, htk=False)).to(device)
        self.conv0 = Conv(sd["input_stack.0.weight"], sd["input_stack.0.bias"], device=device)
        self.gn = (dev("input_stack.1.weight"), dev("input_stack.1.bias"))
        b1 = sd["input_stack.3.bias"]
        if model.get("use_harmonic_emb"):  # forward adds harmonic_emb(0) to every frame when _h_emb is None
            b1 = b1 + sd["harmonic_emb.weight"][0]
        self.conv1 = Conv(sd["input_stack.3.weight"], b1, device=device)
        self.layers = []
        for i in range(self.n_layers):
            p = f"net.encoder_layers.{i}.conformer.net."  # encoder_layers.i.norm.* is the attention branch's: unused
            dw = sd[p + "4.conv.weight"]
            if dw.shape[1] != 1 or dw.shape[2] % 2 == 0 or dw.shape[2] > 31:
                raise NotImplementedError(f"fcpe: depthwise kernel {tuple(dw.shape)}")
            self.layers.append(dict(ln=(dev(p + "0.weight"), dev(p + "0.bias")),
                                    up=Conv(sd[p + "2.weight"], sd[p + "2.bias"], device=device),
                                    dw=(dw[:, 0].contiguous().to(device), dev(p + "4.conv.bias"), int(dw.shape[2])),
                                    down=Conv(sd[p + "6.weight"], sd[p + "6.bias"], device=device)))
        self.norm = (dev("norm.weight"), dev("norm.bias"))
        w = torch._weight_norm(sd["output_proj.parametrizations.weight.original1"],
                               sd["output_proj.parametrizations.weight.original0"], 0)
        self.proj = Conv(w.unsqueeze(-1).contiguous(), sd["output_proj.bias"], device=device)
        self.cent_table = dev("cent_table")
        self._bufs = {}

    @classmethod
    def from_file(cls, path, device="cuda"):
        return cls(torch.load(path, map_location="cpu", weights_only=True), device)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, T, dev):
        """Activation buffers for T frames, allocated once and reused (a captured graph keeps its own)."""
        store = self._bufs if ops._WS_PRIVATE is None else ops._WS_PRIVATE
        key = f"fcpe{id(self)}/{T}/{torch.cuda.current_stream(dev).stream_id}"
        b = store.get(key)
        if b is None:
            C = self.C
            e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
            b = store[key] = dict(mel=e(128, T), a=e(C, T), b=e(C, T), n=e(C, T), h=e(4 * C, T), u=e(2 * C, T),
                                  latent=e(360, T), f0m=e(T))
        return b

    # ------------------------------------------------------------------ network
    def _x32(self, x32):
        if not x32.is_cuda or x32.dtype != torch.float32 or not x32.is_contiguous() or x32.dim() != 1:
            raise TypeError(f"rvc_amd fcpe: expected a contiguous 1-D CUDA f32 signal, got {x32.dtype} "
                            f"{tuple(x32.shape)} on {x32.device}")
        if x32.numel() <= 432:
            raise ValueError(f"fcpe: {x32.numel()} samples (the reference's constant-padding case, at most 432, "
                             "is not supported)")
        return x32.numel() // 160 + 1

    def mel(self, x32, out=None):
        """x32 device f32 [n] at 16 kHz -> log-mel [128][n // 160 + 1]."""
        T = self._x32(x32)
        out = torch.empty(128, T, device=x32.device) if out is None else out
        ops.check(_lib.load().rvc_fcpe_mel(_pv(x32), _pv(self.basis), _pv(out), 1, x32.numel(), ops._stream()),
                  "fcpe_mel")
        return out

    def _latent(self, x32, buf):
        lib, C, T, dev = _lib.load(), self.C, buf["f0m"].numel(), x32.device
        self.mel(x32, buf["mel"])
        with ops.precision(PRECISION):
            self.conv0(buf["mel"], pad=1, out=buf["a"])
            need = lib.rvc_groupnorm_work_bytes(1, 4)
            work = ops._workspace(dev, need, "fcpe_gn")
            ops.check(lib.rvc_groupnorm_act(_pv(buf["a"]), _pv(self.gn[0]), _pv(self.gn[1]), _pv(buf["b"]), 1, C, T, 4,
                                            1e-5, 0.01, _pv(work), need, ops._stream()), "groupnorm_act")
            x, y = buf["a"], buf["b"]
            self.conv1(y, pad=1, out=x)
            for L in self.layers:
                ops.layernorm_cf(x, None, L["ln"][0], L["ln"][1], buf["n"], 1, C, T)
                L["up"](buf["n"], out=buf["h"])
                w, b, K = L["dw"]
                ops.check(lib.rvc_glu_dwconv_silu(_pv(buf["h"]), _pv(w), _pv(b), _pv(buf["u"]), 1, 2 * C, T, K,
                                                  ops._stream()), "glu_dwconv_silu")
                L["down"](buf["u"], out=y, res=x)
                x, y = y, x
            ops.layernorm_cf(x, None, self.norm[0], self.norm[1], buf["n"], 1, C, T)
            self.proj(buf["n"], out=buf["latent"], out_act=ACT_SIGMOID)
        return buf["latent"]

    def latent(self, x32):
        """CFNaiveMelPE.forward's sigmoid output, channels-first [360][n // 160 + 1] (a copy)."""
        return self._latent(x32, self._buffers(self._x32(x32), x32.device)).clone()

    # ------------------------------------------------------------------ f0
    def decode(self, latent, threshold=0.006, f0_min=50, f0_max=1100, out=None):
        """latent device f32 [360][T] -> the model's f0 f32 [T] (0 = unvoiced)."""
        C, T = latent.shape
        out = torch.empty(T, device=latent.device) if out is None else out
        ops.check(_lib.load().rvc_fcpe_decode(_pv(latent), _pv(self.cent_table), _pv(out), 1, C, T, float(threshold),
                                              float(f0_min), float(f0_max), ops._stream()), "fcpe_decode")
        return out

    @staticmethod
    def post(f0m, p_len, hop_length=160, sample_rate=16000):
        """The model's f0 f32 [T] -> compute_f0's return, device f64 [p_len]."""
        lib = _lib.load()
        need = lib.rvc_fcpe_post_work_bytes(int(p_len))
        if need < 0:
            raise ValueError(f"fcpe: bad p_len {p_len}")
        work = ops._workspace(f0m.device, need, "fcpe_post")
        out = torch.empty(int(p_len), dtype=torch.float64, device=f0m.device)
        ops.check(lib.rvc_fcpe_post(_pv(f0m), f0m.numel(), int(p_len), int(hop_length), int(sample_rate), _pv(work),
                                    need, _pv(out), ops._stream()), "fcpe_post")
        return out

    def f0(self, x32, p_len, hop_length=160, threshold=0.006, f0_min=50, f0_max=1100):
        """get_f0_fcpe: x32 device f32 [n] at 16 kHz -> f0 f64 [p_len]."""
        buf = self._buffers(self._x32(x32), x32.device)
        self.decode(self._latent(x32, buf), threshold, f0_min, f0_max, out=buf["f0m"])
        return self.post(buf["f0m"], p_len, hop_length)

    def f0_device(self, xp, pitch, p_len, post=None, hop_length=160, f0_min=50, f0_max=1100):
        """get_f0(..., "fcpe") on the device: (coarse int64 [p_len], pitchf f32 [p_len])."""
        f0 = self.f0(xp, p_len, hop_length, 0.006, f0_min, f0_max)
        coarse = torch.empty(p_len, dtype=torch.int64, device=xp.device)
        pitchf = torch.empty(p_len, dtype=torch.float32, device=xp.device)
        ops.check(_lib.load().rvc_pm_post(_pv(f0), p_len, p_len, float(2.0 ** (pitch / 12)),
                                          ops._post_ref(post, p_len), _pv(coarse), _pv(pitchf), ops._stream()),
                  "pm_post")
        return coarse, pitchf
