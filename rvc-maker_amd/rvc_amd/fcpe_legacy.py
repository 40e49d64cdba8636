"""fcpe-legacy f0 on the device: ``VC.get_f0_fcpe(legacy=True)`` (main/inference/convert.py:239-246) -- the
Performer-attention ``FCPE_LEGACY`` of main/library/predictors/FCPE.py behind ``Wav2Mel``, at 16 kHz and threshold
0.03 -- followed by get_f0's shift / autotune / f0 file / mel quantiser (``rvc_pm_post``).

The mel front end, GroupNorm, the Conformer conv module, the local-argmax decoder and the post-processing are
fcpe's (csrc/fcpe.hip: ``Wav2Mel`` computes what ``Wav2MelModule`` does, bit for bit); what the legacy model adds is
12 layers of FAVOR+ linear self-attention, csrc/performer.hip.  Per layer (``_EncoderLayer.forward``, FCPE.py:387-389):
x + to_out(performer(to_q, to_k, to_v of LayerNorm(x))), then x + conformer(x).  The three input linears are one
1x1 conv C -> 1536 whose output the kernel reads in place, and ``to_out`` takes the residual in its epilogue; the
linears run on the conv engine in f32-accurate arithmetic like every other conv here.  The decoder has no f0 range
(FCPE_LEGACY.forward never clamps; ``load_state_dict`` replaces the constructor's ``cent_table`` with the
checkpoint's): ``rvc_fcpe_decode`` with the range open.  Nothing on the f0 path synchronises with the host.
tests/golden/fcpe_legacy.npz pins the reference's output on synthetic weights.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, melbasis, ops
from .fcpe import PRECISION, FcpeAMD, _pv
from .ops import ACT_SIGMOID, Conv

HEADS, DIM_HEAD = 8, 64  # SelfAttention's defaults (FCPE.py:586): PCmer builds every layer with them
INNER = HEADS * DIM_HEAD
MAX_FEATURES = 272  # RVC_PERFORMER_MAX_FEATURES
F0_OPEN = 3.4028234663852886e38  # FLT_MAX: rvc_fcpe_decode's f0_max when there is no range


def _check_config(cfg, sd):
    model = cfg.get("model") or {}
    if model.get("out_dims", 360) != 360:
        raise NotImplementedError(f"fcpe-legacy: model.out_dims = {model.get('out_dims')}")
    if model.get("input_channel", 128) != 128:
        raise NotImplementedError(f"fcpe-legacy: model.input_channel = {model.get('input_channel')} (the mel front "
                                  "end gives 128)")
    if model.get("confidence"):
        raise NotImplementedError("fcpe-legacy: model.confidence = True (the decoder would return a pair)")
    if model.get("use_input_conv") is False:
        raise NotImplementedError("fcpe-legacy: model.use_input_conv = False")
    for i in range(int(model["n_layers"])):
        shape = tuple(sd[f"decoder._layers.{i}.attn.fast_attention.projection_matrix"].shape)
        if len(shape) != 2 or shape[1] != DIM_HEAD or not 1 <= shape[0] <= MAX_FEATURES:
            raise NotImplementedError(f"fcpe-legacy: layer {i}'s projection_matrix is {shape} (the kernel takes "
                                      f"[1..{MAX_FEATURES}][{DIM_HEAD}])")
    return model


class FcpeLegacyAMD(FcpeAMD):
    def __init__(self, ckpt: dict, device="cuda"):
        model = _check_config(ckpt["config"], ckpt["model"])
        sd = {k: v.float() for k, v in ckpt["model"].items()}
        self.device = device
        self.C, self.n_layers = int(model["n_chans"]), int(model["n_layers"])
        C = self.C
        if sd["stack.0.weight"].shape != (C, 128, 3) or C % 4 or C > 2048:
            raise ValueError(f"fcpe-legacy: n_chans {C} does not match the checkpoint")

        def dev(name):
            return sd[name].contiguous().to(device)

        def linear(names):
            w = torch.cat([sd[n + ".weight"] for n in names])
            return Conv(w.unsqueeze(-1).contiguous(), torch.cat([sd[n + ".bias"] for n in names]), device=device)

        self.basis = torch.from_numpy(melbasis.mel_filterbank(16000, 1024, 128, 0, 8000, htk=False)).to(device)
        self.conv0 = Conv(sd["stack.0.weight"], sd["stack.0.bias"], device=device)
        self.gn = (dev("stack.1.weight"), dev("stack.1.bias"))
        self.conv1 = Conv(sd["stack.3.weight"], sd["stack.3.bias"], device=device)
        self.layers = []
        for i in range(self.n_layers):
            n, a, p = (f"decoder._layers.{i}.{s}" for s in ("norm.", "attn.", "conformer.net."))
            dw = sd[p + "4.conv.weight"]
            if dw.shape[1] != 1 or dw.shape[2] % 2 == 0 or dw.shape[2] > 31:
                raise NotImplementedError(f"fcpe-legacy: depthwise kernel {tuple(dw.shape)}")
            if sd[a + "to_q.weight"].shape != (INNER, C):
                raise NotImplementedError(f"fcpe-legacy: to_q {tuple(sd[a + 'to_q.weight'].shape)} ({HEADS} heads of "
                                          f"{DIM_HEAD} are on the MI355X path)")
            self.layers.append(dict(norm=(dev(n + "weight"), dev(n + "bias")),
                                    qkv=linear([a + "to_q", a + "to_k", a + "to_v"]),
                                    proj=dev(a + "fast_attention.projection_matrix"),
                                    to_out=linear([a + "to_out"]),
                                    ln=(dev(p + "0.weight"), dev(p + "0.bias")),
                                    up=Conv(sd[p + "2.weight"], sd[p + "2.bias"], device=device),
                                    dw=(dw[:, 0].contiguous().to(device), dev(p + "4.conv.bias"), int(dw.shape[2])),
                                    down=Conv(sd[p + "6.weight"], sd[p + "6.bias"], device=device)))
        self.norm = (dev("norm.weight"), dev("norm.bias"))
        w = torch._weight_norm(sd["dense_out.parametrizations.weight.original1"],
                               sd["dense_out.parametrizations.weight.original0"], 0)
        self.proj = Conv(w.unsqueeze(-1).contiguous(), sd["dense_out.bias"], device=device)
        self.cent_table = dev("cent_table")
        self._bufs = {}

    # ------------------------------------------------------------------ buffers
    def _buffers(self, T, dev):
        store = self._bufs if ops._WS_PRIVATE is None else ops._WS_PRIVATE
        key = f"fcpe_legacy{id(self)}/{T}/{torch.cuda.current_stream(dev).stream_id}"
        b = store.get(key)
        if b is None:
            C = self.C
            e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
            b = store[key] = dict(mel=e(128, T), a=e(C, T), b=e(C, T), n=e(C, T), h=e(4 * C, T), u=e(2 * C, T),
                                  qkv=e(3 * INNER, T), att=e(INNER, T), latent=e(360, T), f0m=e(T))
        return b

    # ------------------------------------------------------------------ network
    @staticmethod
    def performer(qkv, proj, out):
        """qkv device f32 [3 * 512][T] (to_q, to_k, to_v stacked), proj [M][64] -> out [512][T]."""
        lib, T, M = _lib.load(), qkv.shape[1], proj.shape[0]
        need = lib.rvc_performer_work_bytes(1, HEADS, T, M)
        if need < 0:
            raise ValueError(f"fcpe-legacy: bad attention shape T={T} M={M}")
        work = ops._workspace(qkv.device, need, "performer")
        step = INNER * T * 4
        ops.check(lib.rvc_performer_attention(_pv(qkv), ctypes.c_void_p(qkv.data_ptr() + step),
                                              ctypes.c_void_p(qkv.data_ptr() + 2 * step), _pv(proj), _pv(out), 1, HEADS,
                                              T, DIM_HEAD, M, T, 3 * INNER * T, INNER * T, _pv(work), need,
                                              ops._stream()), "performer_attention")
        return out

    def self_attention(self, L, n, buf, out, res=None):
        """SelfAttention.forward on n [C][T] (the layer's LayerNorm output): out = to_out(performer(to_q, to_k,
        to_v of n)) (+ res)."""
        L["qkv"](n, out=buf["qkv"])
        self.performer(buf["qkv"], L["proj"], buf["att"])
        return L["to_out"](buf["att"], out=out, res=res)

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
                ops.layernorm_cf(x, None, L["norm"][0], L["norm"][1], buf["n"], 1, C, T)
                self.self_attention(L, buf["n"], buf, y, res=x)
                x, y = y, x
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

    # ------------------------------------------------------------------ f0
    def decode(self, latent, threshold=0.03, out=None):
        """latent device f32 [360][T] -> the model's f0 f32 [T] (0 = unvoiced): confidence <= threshold -> 0 and no
        f0 range."""
        return super().decode(latent, threshold, 0.0, F0_OPEN, out=out)

    def f0(self, x32, p_len, hop_length=160, threshold=0.03):
        """get_f0_fcpe(legacy=True): x32 device f32 [n] at 16 kHz -> f0 f64 [p_len]."""
        buf = self._buffers(self._x32(x32), x32.device)
        self.decode(self._latent(x32, buf), threshold, out=buf["f0m"])
        return self.post(buf["f0m"], p_len, hop_length)

    def f0_device(self, xp, pitch, p_len, post=None, hop_length=160):
        """get_f0(..., "fcpe-legacy") on the device: (coarse int64 [p_len], pitchf f32 [p_len])."""
        f0 = self.f0(xp, p_len, hop_length, 0.03)
        coarse = torch.empty(p_len, dtype=torch.int64, device=xp.device)
        pitchf = torch.empty(p_len, dtype=torch.float32, device=xp.device)
        ops.check(_lib.load().rvc_pm_post(_pv(f0), p_len, p_len, float(2.0 ** (pitch / 12)),
                                          ops._post_ref(post, p_len), _pv(coarse), _pv(pitchf), ops._stream()),
                  "pm_post")
        return coarse, pitchf
