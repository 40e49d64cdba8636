"""fcpe f0 on the device: ``VC.get_f0_fcpe`` (main/inference/convert.py:239-246) -- the conv-only
``CFNaiveMelPE`` of main/library/predictors/FCPE.py at 16 kHz, threshold 0.006, 50..1100 Hz -- followed by
get_f0's shift / autotune / f0 file / mel quantiser (convert.py:308-323, ``ops.f0_post64``).

The mel front end, GroupNorm, the Conformer block's GLU / depthwise conv / SiLU, the local-argmax decoder and
the post-processing are csrc/fcpe.hip; the dense convs run on the conv engine in f32-accurate arithmetic (the
6-pass split-bf16 form: f0 is a per-frame argmax and threshold decision) and the LayerNorms are
``rvc_layernorm_cf``.  Nothing on the f0 path synchronises with the host.  tests/golden/fcpe.npz pins the
reference's output on synthetic weights; tests/fcpe_ref.py restates the decode and post stages in numpy.

``FcpeAMD`` is cut into the pieces ``fcpe_legacy.FcpeLegacyAMD`` reuses: the class-level table of checkpoint names,
``_conformer_weights``, ``_stem``, ``_conformer``, ``_head``, ``_buffers`` (with ``_extra_buffers``) and the class's
``THRESHOLD``; a subclass overrides ``_layer_weights`` / ``_layer`` for what its encoder layer adds.
"""
from __future__ import annotations

import torch

from . import _lib, melbasis, ops
from .ops import ACT_SIGMOID, Conv, _p

GLU_TILE = 256  # RVC_GLU_DW_TILE
PRECISION = "fp32x6"
MEL_GEOMETRY = {"num_mels": 128, "n_fft": 1024, "win_size": 1024, "hop_size": 160, "fmin": 0, "fmax": 8000}
MEL_DEFAULTS = dict(MEL_GEOMETRY, sr=16000)  # spawn_wav2mel's defaults for absent fields (FCPE.py:153)


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
    # where the checkpoint keeps what: config key, the config field of the channel count, the prefixes of the stem,
    # of layer i and of the output projection (FcpeLegacyAMD: the same modules under FCPE_LEGACY's names)
    NAME, CONFIG, CHANS = "fcpe", "config_dict", "hidden_dims"
    STEM, LAYER, OUT = "input_stack.", "net.encoder_layers.{}.", "output_proj."
    THRESHOLD = 0.006  # get_f0_fcpe's confidence threshold for this model

    def __init__(self, ckpt: dict, device="cuda"):
        model = self._check_config(ckpt[self.CONFIG], ckpt["model"])
        sd = {k: v.float() for k, v in ckpt["model"].items()}
        self.device = device
        self.C, self.n_layers = int(model[self.CHANS]), int(model["n_layers"])
        C, S = self.C, self.STEM
        if sd[S + "0.weight"].shape != (C, 128, 3) or C % 4 or C > 2048:
            raise ValueError(f"{self.NAME}: {self.CHANS} {C} does not match the checkpoint")
        self.basis = torch.from_numpy(melbasis.mel_filterbank(16000, 1024, 128, 0, 8000, htk=False)).to(device)
        self.conv0 = Conv(sd[S + "0.weight"], sd[S + "0.bias"], device=device)
        self.gn = (self._dev(sd, S + "1.weight"), self._dev(sd, S + "1.bias"))
        b1 = sd[S + "3.bias"]
        if model.get("use_harmonic_emb"):  # forward adds harmonic_emb(0) to every frame when _h_emb is None
            b1 = b1 + sd["harmonic_emb.weight"][0]
        self.conv1 = Conv(sd[S + "3.weight"], b1, device=device)
        self.layers = [self._layer_weights(sd, self.LAYER.format(i)) for i in range(self.n_layers)]
        self.norm = (self._dev(sd, "norm.weight"), self._dev(sd, "norm.bias"))
        w = torch._weight_norm(sd[self.OUT + "parametrizations.weight.original1"],
                               sd[self.OUT + "parametrizations.weight.original0"], 0)
        self.proj = Conv(w.unsqueeze(-1).contiguous(), sd[self.OUT + "bias"], device=device)
        self.cent_table = self._dev(sd, "cent_table")
        self._bufs = {}

    @staticmethod
    def _check_config(cfg, sd):
        return _check_config(cfg)

    def _dev(self, sd, name):
        return sd[name].contiguous().to(self.device)

    def _layer_weights(self, sd, prefix):
        # encoder_layers.i.norm.* is the attention branch's: unused when conv_only
        return self._conformer_weights(sd, prefix + "conformer.net.")

    def _conformer_weights(self, sd, p):
        """One layer's Conformer conv module: LayerNorm, 1x1 up, GLU + depthwise conv + SiLU, 1x1 down."""
        dw = sd[p + "4.conv.weight"]
        if dw.shape[1] != 1 or dw.shape[2] % 2 == 0 or dw.shape[2] > 31:
            raise NotImplementedError(f"{self.NAME}: depthwise kernel {tuple(dw.shape)}")
        return dict(ln=(self._dev(sd, p + "0.weight"), self._dev(sd, p + "0.bias")),
                    up=Conv(sd[p + "2.weight"], sd[p + "2.bias"], device=self.device),
                    dw=(dw[:, 0].contiguous().to(self.device), self._dev(sd, p + "4.conv.bias"), int(dw.shape[2])),
                    down=Conv(sd[p + "6.weight"], sd[p + "6.bias"], device=self.device))

    @classmethod
    def from_file(cls, path, device="cuda"):
        return cls(torch.load(path, map_location="cpu", weights_only=True), device)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, T, dev):
        """Activation buffers for T frames, allocated once and reused (a captured graph keeps its own)."""
        store = self._bufs if ops._WS_PRIVATE is None else ops._WS_PRIVATE
        key = f"{self.NAME.replace('-', '_')}{id(self)}/{T}/{torch.cuda.current_stream(dev).stream_id}"
        b = store.get(key)
        if b is None:
            C = self.C
            shapes = dict(mel=(128, T), a=(C, T), b=(C, T), n=(C, T), h=(4 * C, T), u=(2 * C, T), latent=(360, T),
                          f0m=(T,), **self._extra_buffers(T))
            b = store[key] = {k: torch.empty(*s, device=dev) for k, s in shapes.items()}
        return b

    def _extra_buffers(self, T):
        return {}

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
        ops.check(_lib.load().rvc_fcpe_mel(_p(x32), _p(self.basis), _p(out), 1, x32.numel(), ops._stream()),
                  "fcpe_mel")
        return out

    def _stem(self, x32, buf):
        """mel, conv, GroupNorm + LeakyReLU, conv -> (x, y): the stem's output and the layers' other ping-pong
        buffer."""
        lib, C, T = _lib.load(), self.C, buf["f0m"].numel()
        self.mel(x32, buf["mel"])
        self.conv0(buf["mel"], pad=1, out=buf["a"])
        need = lib.rvc_groupnorm_work_bytes(1, 4)
        work = ops._workspace(x32.device, need, "fcpe_gn")
        ops.check(lib.rvc_groupnorm_act(_p(buf["a"]), _p(self.gn[0]), _p(self.gn[1]), _p(buf["b"]), 1, C, T, 4, 1e-5,
                                        0.01, _p(work), need, ops._stream()), "groupnorm_act")
        self.conv1(buf["b"], pad=1, out=buf["a"])
        return buf["a"], buf["b"]

    def _conformer(self, L, x, y, buf):
        """y = x + conformer(x) (ConformerConvModule) -> (y, x), the buffers swapped."""
        C, T = x.shape
        ops.layernorm_cf(x, None, L["ln"][0], L["ln"][1], buf["n"], 1, C, T)
        L["up"](buf["n"], out=buf["h"])
        w, b, K = L["dw"]
        ops.check(_lib.load().rvc_glu_dwconv_silu(_p(buf["h"]), _p(w), _p(b), _p(buf["u"]), 1, 2 * C, T, K,
                                                  ops._stream()), "glu_dwconv_silu")
        L["down"](buf["u"], out=y, res=x)
        return y, x

    _layer = _conformer  # one encoder layer: here the conformer alone

    def _head(self, x, buf):
        """The final LayerNorm and the sigmoid output projection -> buf["latent"]."""
        C, T = x.shape
        ops.layernorm_cf(x, None, self.norm[0], self.norm[1], buf["n"], 1, C, T)
        self.proj(buf["n"], out=buf["latent"], out_act=ACT_SIGMOID)
        return buf["latent"]

    def _latent(self, x32, buf):
        with ops.precision(PRECISION):  # the convs' arithmetic (the mel kernel does not read it)
            x, y = self._stem(x32, buf)
            for L in self.layers:
                x, y = self._layer(L, x, y, buf)
            return self._head(x, buf)

    def latent(self, x32):
        """CFNaiveMelPE.forward's sigmoid output, channels-first [360][n // 160 + 1] (a copy)."""
        return self._latent(x32, self._buffers(self._x32(x32), x32.device)).clone()

    # ------------------------------------------------------------------ f0
    def decode(self, latent, threshold=0.006, f0_min=50, f0_max=1100, out=None):
        """latent device f32 [360][T] -> the model's f0 f32 [T] (0 = unvoiced)."""
        C, T = latent.shape
        out = torch.empty(T, device=latent.device) if out is None else out
        ops.check(_lib.load().rvc_fcpe_decode(_p(latent), _p(self.cent_table), _p(out), 1, C, T, float(threshold),
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
        ops.check(lib.rvc_fcpe_post(_p(f0m), f0m.numel(), int(p_len), int(hop_length), int(sample_rate), _p(work),
                                    need, ops._pd(out), ops._stream()), "fcpe_post")
        return out

    def f0(self, x32, p_len, hop_length=160, threshold=0.006, f0_min=50, f0_max=1100):
        """get_f0_fcpe: x32 device f32 [n] at 16 kHz -> f0 f64 [p_len]."""
        buf = self._buffers(self._x32(x32), x32.device)
        self.decode(self._latent(x32, buf), threshold, f0_min, f0_max, out=buf["f0m"])
        return self.post(buf["f0m"], p_len, hop_length)

    def f0_device(self, xp, pitch, p_len, post=None, hop_length=160, f0_min=50, f0_max=1100):
        """get_f0(..., "fcpe" / "fcpe-legacy") on the device: (coarse int64 [p_len], pitchf f32 [p_len])."""
        return ops.f0_post64(self.f0(xp, p_len, hop_length, self.THRESHOLD, f0_min, f0_max), p_len, pitch, post)
