"""fcpe-legacy f0 on the device: ``VC.get_f0_fcpe(legacy=True)`` (main/inference/convert.py:239-246) -- the
Performer-attention ``FCPE_LEGACY`` of main/library/predictors/FCPE.py behind ``Wav2Mel``, at 16 kHz and threshold
0.03 -- followed by get_f0's shift / autotune / f0 file / mel quantiser (``ops.f0_post64``).

The mel front end, GroupNorm, the Conformer conv module, the local-argmax decoder and the post-processing are
fcpe's (csrc/fcpe.hip: ``Wav2Mel`` computes what ``Wav2MelModule`` does, bit for bit), and so is the code that runs
them: ``FcpeLegacyAMD`` is ``FcpeAMD`` with FCPE_LEGACY's checkpoint names, its config checks, the attention weights
and buffers, the layer order and the open f0 range; constructor, stem, conformer, head and ``f0_device`` are
inherited.  What the legacy model adds is
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

from . import _lib, ops
from .fcpe import FcpeAMD
from .ops import Conv, _p

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
    NAME, CONFIG, CHANS = "fcpe-legacy", "config", "n_chans"
    STEM, LAYER, OUT = "stack.", "decoder._layers.{}.", "dense_out."
    THRESHOLD = 0.03

    _check_config = staticmethod(_check_config)

    def _layer_weights(self, sd, prefix):
        n, a = prefix + "norm.", prefix + "attn."
        if sd[a + "to_q.weight"].shape != (INNER, self.C):
            raise NotImplementedError(f"fcpe-legacy: to_q {tuple(sd[a + 'to_q.weight'].shape)} ({HEADS} heads of "
                                      f"{DIM_HEAD} are on the MI355X path)")

        def linear(names):
            w = torch.cat([sd[a + k + ".weight"] for k in names])
            return Conv(w.unsqueeze(-1).contiguous(), torch.cat([sd[a + k + ".bias"] for k in names]),
                        device=self.device)

        return dict(self._conformer_weights(sd, prefix + "conformer.net."),
                    norm=(self._dev(sd, n + "weight"), self._dev(sd, n + "bias")),
                    qkv=linear(["to_q", "to_k", "to_v"]), to_out=linear(["to_out"]),
                    proj=self._dev(sd, a + "fast_attention.projection_matrix"))

    def _extra_buffers(self, T):
        return dict(qkv=(3 * INNER, T), att=(INNER, T))

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
        ops.check(lib.rvc_performer_attention(_p(qkv), ctypes.c_void_p(qkv.data_ptr() + step),
                                              ctypes.c_void_p(qkv.data_ptr() + 2 * step), _p(proj), _p(out), 1, HEADS,
                                              T, DIM_HEAD, M, T, 3 * INNER * T, INNER * T, _p(work), need,
                                              ops._stream()), "performer_attention")
        return out

    def self_attention(self, L, n, buf, out, res=None):
        """SelfAttention.forward on n [C][T] (the layer's LayerNorm output): out = to_out(performer(to_q, to_k,
        to_v of n)) (+ res)."""
        L["qkv"](n, out=buf["qkv"])
        self.performer(buf["qkv"], L["proj"], buf["att"])
        return L["to_out"](buf["att"], out=out, res=res)

    def _layer(self, L, x, y, buf):
        """_EncoderLayer.forward (FCPE.py:387-389): x + attention(LayerNorm(x)), then x + conformer(x)."""
        C, T = x.shape
        ops.layernorm_cf(x, None, L["norm"][0], L["norm"][1], buf["n"], 1, C, T)
        self.self_attention(L, buf["n"], buf, y, res=x)
        return self._conformer(L, y, x, buf)

    # ------------------------------------------------------------------ f0
    def decode(self, latent, threshold=0.03, out=None):
        """latent device f32 [360][T] -> the model's f0 f32 [T] (0 = unvoiced): confidence <= threshold -> 0 and no
        f0 range."""
        return super().decode(latent, threshold, 0.0, F0_OPEN, out=out)

    def f0(self, x32, p_len, hop_length=160, threshold=0.03, f0_min=None, f0_max=None):
        """get_f0_fcpe(legacy=True): x32 device f32 [n] at 16 kHz -> f0 f64 [p_len].  ``f0_min`` / ``f0_max`` are taken
        as the reference's FCPE(legacy=True) takes them and, as there, never read."""
        buf = self._buffers(self._x32(x32), x32.device)
        self.decode(self._latent(x32, buf), threshold, out=buf["f0m"])
        return self.post(buf["f0m"], p_len, hop_length)
